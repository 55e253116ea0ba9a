"""The host reference of the input transform (oracle/dib_oracle.py A23: plain numpy, no torch, nothing of the package) pinned on the
CPU: its real-arithmetic positions against torch's float64 F.interpolate, its restated float32 positions against the reference's
own float32 goldens (tests/golden/net_transforms.npz) and torch's float32 interpolate through the one comparison function, its
quantisation against GeneralizedRCNNTransform.quantize over every Half of the domain -- and the comparison function itself against a
numpy float32 emulation of the kernel: as written it passes, with any one of eight single defects it does not.

This module also builds the inputs (numpy) that both halves use; tests/test_input_transform_f64_gpu.py feeds them to the HIP
kernels."""
import os

import numpy as np
import pytest
import torch

import dib_oracle as O
import gen_goldens as GG

F = torch.nn.functional
INF, NAN = float("inf"), float("nan")
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "net_transforms.npz"))

# ((H, W), (Ho, Wo)) per image of a batch; the batch extent; crop or pad
RESIZE_PAD = dict(Hp=96, Wp=320, crop=False, sizes=[
    ((5, 7), (32, 45)),            # upscale
    ((37, 53), (64, 91)),          # upscale
    ((70, 100), (33, 47)),         # downscale past 2x
    ((3, 1), (96, 32)),            # width of 1
    ((2, 2), (7, 5)),              # tiny source
    ((1, 5), (1, 9)),              # height identity
    ((9, 260), (9, 300)),          # one-axis identity; crosses the 256-column block
    ((40, 30), (13, 90)),          # down on one axis, up on the other (aspect-distorting)
    ((64, 96), (64, 96))])         # unit scale inside a resizing batch
CROP_32 = dict(Hp=32, Wp=32, crop=True, sizes=[
    ((128, 200), (32, 48)),        # resized height == the crop; at 4x the last output row reads source rows 125 and 126
    ((40, 70), (40, 70)), ((33, 40), (64, 78)),
    ((50, 77), (32, 49)),          # ... at 1.5625x it reads rows 48 and 49: the last source row, with a step (ip = 1)
    ((20, 25), (32, 40)),          # ... and upscaled it reads row 19 alone: the last source row behind the edge clamp (ip = 0)
    ((9, 11), (45, 33))])
CROP_288 = dict(Hp=32, Wp=288, crop=True, sizes=[((96, 300), (96, 300)), ((100, 330), (33, 290)), ((20, 150), (40, 300))])
UNIT = dict(Hp=32, Wp=288, crop=False, sizes=[(s, s) for s in ((5, 7), (32, 32), (1, 1), (3, 260), (31, 257))])
# 33 images (one more than a launch takes) with DISTINCT statistics per image: a wrong chunk offset is a wrong value
BATCH33 = {"unit": dict(Hp=8, Wp=8, crop=False, sizes=[((4, 6), (4, 6))] * 33),
           "resize": dict(Hp=8, Wp=12, crop=False, sizes=[((4, 6), (7, 9))] * 33),
           "crop": dict(Hp=5, Wp=8, crop=True, sizes=[((4, 6), (7, 9))] * 33)}
QUANT = {"pad": dict(Hp=32, Wp=64, crop=False, sizes=[((20, 40), (20, 40))] * 2),
         "pad_resize": dict(Hp=32, Wp=64, crop=False, sizes=[((20, 40), (31, 55)), ((20, 40), (20, 40))]),
         "crop": dict(Hp=16, Wp=32, crop=True, sizes=[((20, 40), (20, 40))] * 2),
         "crop_resize": dict(Hp=16, Wp=32, crop=True, sizes=[((20, 40), (31, 55)), ((20, 40), (24, 47))])}
LAYOUTS = {"resize_pad": RESIZE_PAD, "crop_32": CROP_32, "crop_288": CROP_288, "unit": UNIT}


def salt(img):
    """NaN, +-inf, Half's largest value, Half's smallest denormal and -0 (float32 images: float32's smallest denormal and a value
    that overflows under normalisation as well) in a corner, on the last row and the last column, and in the interior."""
    H, W = img.shape[1:]
    if H < 5 or W < 7:
        return img
    img[0, 0, 0] = NAN                                    # corner
    img[1, H - 1, W - 1] = INF                            # the other corner: last row and last column
    img[2, H // 2, W // 2] = -INF                         # interior
    img[0, H - 1, W // 2] = 65504.0                       # last row
    img[1, H // 2, W - 1] = 2.0 ** -24                    # last column
    img[2, 1, 2] = -0.0
    img[0, H // 2, 1] = -0.0
    if img.dtype == np.float32:
        img[1, 2, 3] = 1e-45
        img[2, H - 1, 0] = 3e38
    return img


def statistics(B, seed):
    """float64 rows, not float32 numbers; image 1 has mean 0 (a -0.0 pixel stays -0.0) and power-of-two stds"""
    rs = np.random.RandomState(seed)
    means, stds = rs.uniform(0.3, 0.6, (B, 3)), rs.uniform(0.1, 0.3, (B, 3))
    if B > 1:
        means[1], stds[1] = 0.0, (1.0, 0.5, 0.25)
    return means, stds


def build(layout, dtype, seed, specials=True):
    """A case: the arguments of O.input_transform64 as a dict."""
    rs = np.random.RandomState(seed)
    images = []
    for (H, W), _ in layout["sizes"]:
        img = rs.random_sample((3, H, W)).astype(dtype)
        images.append(salt(img) if specials else img)
    means, stds = statistics(len(images), seed + 1)
    return dict(images=images, means=means, stds=stds, out_sizes=[o for _, o in layout["sizes"]], Hp=layout["Hp"], Wp=layout["Wp"],
                crop=layout["crop"], quantize=False)


def build33(kind, dtype):
    case = build(BATCH33[kind], dtype, 33, specials=False)
    k = np.arange(33).reshape(-1, 1)
    case["means"], case["stds"] = 0.3 + 0.01 * k + [[0.0, 0.001, 0.002]], 0.2 + 0.005 * k + [[0.0, 0.0005, 0.001]]
    return case


def quantise_domain_values():
    """every k / 255 as a Half, its two Half neighbours, and on up to 1.0029 (0x3C03), where half(x * 255) is still < 256"""
    k = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float16).view(np.uint16).astype(np.int32)
    bits = np.unique(np.concatenate([k - 1, k, k + 1, np.arange(0x3C00, 0x3C04)]))
    return bits[bits >= 0].astype(np.uint16).view(np.float16)


def build_quant(kind):
    vals = quantise_domain_values()
    assert 765 <= len(vals) <= 800
    layout = QUANT[kind]
    images = [np.stack([np.resize(np.roll(vals, 101 * c + 37 * j), 800).reshape(20, 40) for c in range(3)]) for j in range(2)]
    means, stds = statistics(2, 77)
    return dict(images=images, means=means, stds=stds, out_sizes=[o for _, o in layout["sizes"]], Hp=layout["Hp"], Wp=layout["Wp"],
                crop=layout["crop"], quantize=True)


def ramp_image(H, W, dtype):
    """p[y][x] = (x + 3 y) / 2048 on all three planes: exact in Half for x + 3 y < 2048"""
    p = (np.arange(W, dtype=np.float64)[None, :] + 3.0 * np.arange(H, dtype=np.float64)[:, None]) / 2048.0
    assert p.max() < 1.0 and np.array_equal(p.astype(np.float16).astype(np.float64), p)
    return np.stack([p, p, p]).astype(dtype)


def reference(case, contracted=True):
    return O.input_transform64(case["images"], case["means"], case["stds"], case["out_sizes"], case["Hp"], case["Wp"], case["crop"],
                               case["quantize"], contracted)


# ---- a numpy float32 emulation of the kernel, with single defects ------------------------------------------------------------------

def _fmaf(a, b, c):
    """fmaf for float32 operands: a * b is exact in float64"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _emulate_axis(n_in, n_out, fma, defect):
    f32 = np.float32
    scale = f32(n_in) / f32(n_out)
    t = np.arange(n_out, dtype=np.float32) + (f32(0.0) if defect == "no_half" else f32(0.5))
    s = _fmaf(np.full_like(t, scale), t, np.full_like(t, -0.5)) if fma else scale * t - f32(0.5)
    s = np.where(s < 0, f32(0), s).astype(np.float32)
    i = s.astype(np.int32)
    ip = (i < n_in - 1).astype(np.int32)
    l1 = s - i.astype(np.float32)
    return i, ip, f32(1.0) - l1, l1


def emulate(case, fma=True, defect=None):
    """normalize_resize_pad_kernel (and, for a batch without a resize, normalize_pad_kernel) in numpy float32, launch chunks of
    32 images included.  `defect`: one of DEFECTS, or None for the kernel as written."""
    f32 = np.float32
    B, Hp, Wp = len(case["images"]), case["Hp"], case["Wp"]
    mean = np.asarray(case["means"], dtype=np.float64).reshape(B, 3).astype(np.float32)
    std = np.asarray(case["stds"], dtype=np.float64).reshape(B, 3).astype(np.float32)
    out = np.full((B, 3, Hp, Wp), f32(-0.0) if defect == "negative_zero_padding" else f32(0.0), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for b0 in range(0, B, 32):
            for k in range(b0, min(B, b0 + 32)):
                ks = k - 32 if defect == "chunk_statistics" and k >= 32 else k
                p = case["images"][k]
                H, W = p.shape[1:]
                Ho, Wo = case["out_sizes"][k]
                if case["quantize"]:
                    a = (p.astype(np.float32) * f32(255)).astype(np.float16).astype(np.float32)
                    q = np.rint(a) if defect == "quantise_to_nearest" else np.trunc(a)
                    p = (q.astype(np.uint8).astype(np.float32) / f32(255)).astype(np.float16)
                ch = [(c + 1) % 3 for c in range(3)] if defect == "channel_statistics" else [0, 1, 2]
                n = (p.astype(np.float32) - mean[ks][ch].reshape(3, 1, 1)) / std[ks][ch].reshape(3, 1, 1)
                if (Ho, Wo) != (H, W):
                    h, hp, l0h, l1h = _emulate_axis(H, Ho, fma, defect)
                    w, wp, l0w, l1w = _emulate_axis(W, Wo, fma, defect)
                    if defect == "weights_swapped":
                        l0w, l1w = l1w, l0w
                    if defect == "edge_clamp_ignored":
                        hp = np.zeros_like(hp)
                    l0h, l1h, l0w, l1w = l0h.reshape(-1, 1), l1h.reshape(-1, 1), l0w.reshape(1, -1), l1w.reshape(1, -1)
                    p00, p01, p10 = n[:, h][:, :, w], n[:, h][:, :, w + wp], n[:, h + hp][:, :, w]
                    p11 = p10 if defect == "p11_without_w1p" else n[:, h + hp][:, :, w + wp]
                    shape = p00.shape
                    if fma:
                        l0w, l1w = np.broadcast_to(l0w, shape), np.broadcast_to(l1w, shape)
                        top, bot = _fmaf(l0w, p00, l1w * p01), _fmaf(l0w, p10, l1w * p11)
                        n = _fmaf(np.broadcast_to(l0h, shape), top, l1h * bot)
                    else:
                        n = l0h * (l0w * p00 + l1w * p01) + l1h * (l0w * p10 + l1w * p11)
                hh, ww = min(Ho, Hp), min(Wo, Wp)
                out[k, :, :hh, :ww] = n[:, :hh, :ww]
    return out


# the defect, and the case that has to notice it
DEFECTS = {
    "no_half": lambda: build(RESIZE_PAD, np.float32, 1),                       # `+ 0.5` dropped from the destination index
    "weights_swapped": lambda: build(RESIZE_PAD, np.float16, 1),               # l0w and l1w swapped
    "p11_without_w1p": lambda: build(CROP_32, np.float32, 2),                  # the w1p step missing from p11
    "channel_statistics": lambda: build(UNIT, np.float16, 4),                  # channel c with the statistics of channel (c + 1) % 3
    "chunk_statistics": lambda: build33("resize", np.float32),                 # images >= 32 with the statistics of image k - 32
    "quantise_to_nearest": lambda: build_quant("pad_resize"),                  # rounding instead of truncation
    "negative_zero_padding": lambda: build(UNIT, np.float32, 4),               # padding written as -0.0
    "edge_clamp_ignored": lambda: build(CROP_288, np.float16, 3),              # the row at i repeated instead of i + ip
}
PEAKS = {}


def all_cases():
    for name, layout in LAYOUTS.items():
        for dtype in (np.float16, np.float32):
            yield "%s/%s" % (name, np.dtype(dtype).name), build(layout, dtype, 1 + len(name))
    for kind in BATCH33:
        yield "batch33/" + kind, build33(kind, np.float32)
    for kind in QUANT:
        yield "quantise/" + kind, build_quant(kind)


@pytest.mark.parametrize("fma", [True, False])
def test_the_emulated_kernel_as_written_passes_the_comparison(fma):
    peak = 0.0
    for name, case in all_cases():
        units = O.input_transform_compare(emulate(case, fma), *reference(case, contracted=fma))
        print("%-24s %s: peak %.2f x 2^-24 M" % (name, "contracted" if fma else "uncontracted", units))
        peak = max(peak, units)
    print("CPU emulation, %s: peak %.2f x 2^-24 M over all cases" % ("contracted" if fma else "uncontracted", peak))
    assert 0.0 < peak <= O.TRANSFORM_BOUND


@pytest.mark.parametrize("fma", [True, False])
@pytest.mark.parametrize("defect", list(DEFECTS))
def test_the_comparison_rejects_a_kernel_with_one_defect(defect, fma):
    case = DEFECTS[defect]()
    ref = reference(case, contracted=fma)
    O.input_transform_compare(emulate(case, fma), *ref)                         # the case itself is fine
    with pytest.raises(AssertionError):
        O.input_transform_compare(emulate(case, fma, defect), *ref)


def test_the_two_position_forms_are_two_references():
    """The uncontracted kernel rounds scale * (dst + 0.5) before it subtracts 0.5: its position differs from the contracted one by
    up to half an ulp of the INDEX, which moves the value by that much of the local contrast -- far more than the interpolation's
    own roundings.  So the bound holds against the form the kernel was built with, and not against the other one."""
    case = build(RESIZE_PAD, np.float32, 1)
    for fma in (True, False):
        O.input_transform_compare(emulate(case, fma), *reference(case, contracted=fma))
        with pytest.raises(AssertionError, match="beyond"):
            O.input_transform_compare(emulate(case, fma), *reference(case, contracted=not fma))
    a, b = O.transform_positions(260, 300, True), O.transform_positions(260, 300, False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[4], b[4]) and 0 < np.abs(a[3] - b[3]).max() <= 2.0 ** -16


def test_the_comparison_limits_the_share_of_non_finite_reference_elements():
    case = build(UNIT, np.float32, 4)
    case["images"][1][:, :12, :] = NAN                                          # 3 * 12 * 32 of 5 * 3 * 32 * 288 elements: fine
    O.input_transform_compare(emulate(case), *reference(case))
    for img in case["images"]:
        img[...] = INF                                                          # every image pixel: 21 % of the padded batch
    with pytest.raises(AssertionError, match="not finite"):
        O.input_transform_compare(emulate(case), *reference(case))


def test_the_specials_reach_every_class_and_the_cases_hold_what_they_claim():
    for dtype in (np.float16, np.float32):
        case = build(RESIZE_PAD, dtype, 11)
        v, M, exact = reference(case)
        with np.errstate(over="ignore"):
            v32 = v.astype(np.float32)
        assert np.isnan(v32).any() and (v32 == INF).any() and (v32 == -INF).any()
        assert np.isnan(v32[~exact]).any() and (v32[~exact] == INF).any() and np.isnan(v32[8]).any()       # interpolated and unit scale
        assert exact[8, :, :64, :96].all() and not exact[0, :, :32, :45].any() and exact[0, :, 32:, :].all()
    v, _, exact = reference(build(UNIT, np.float32, 4))
    assert exact.all() and np.signbit(v[v == 0]).any() and not np.signbit(v[:, :, :, 270:]).any()
    n = O.transform_normalize(build(RESIZE_PAD, np.float32, 11)["images"][1], [0.4] * 3, [0.2] * 3)
    assert n.dtype == np.float32 and n[2, 36, 0] == INF                         # 3e38 overflows under normalisation
    # the crops whose resized height equals the crop read the last source row, with and without a step
    i, ip, _, _, _ = O.transform_positions(50, 32)
    assert (i[-1], ip[-1]) == (48, 1)
    i, ip, _, l1, _ = O.transform_positions(20, 32)
    assert (i[-1], ip[-1]) == (19, 0) and l1[-1] > 0


# ---- the reference against torch on the CPU --------------------------------------------------------------------------------------

SHAPES = [s for s in RESIZE_PAD["sizes"] if s[0] != s[1]] + CROP_32["sizes"][:1] + CROP_288["sizes"][1:] + [((480, 640), (800, 1066))]


def test_real_arithmetic_positions_equal_torchs_float64_interpolate():
    for k, ((H, W), (Ho, Wo)) in enumerate(SHAPES):
        img = np.random.RandomState(k).random_sample((3, H, W)).astype(np.float32)
        n = O.transform_normalize(img, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]).astype(np.float64)
        want = F.interpolate(torch.from_numpy(n)[None], size=(Ho, Wo), mode="bilinear", align_corners=False)[0].numpy()
        got = O.transform_bilinear_real64(n, Ho, Wo)
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12, ((H, W), (Ho, Wo), np.abs(got - want).max())
        for n_in, n_out in ((H, Ho), (W, Wo)):
            s = O.transform_positions(n_in, n_out)[4]
            assert s.dtype == np.float64 and s.min() >= 0 and s.max() <= n_in - 1 and (np.diff(s) >= 0).all()


def test_restated_positions_pass_the_comparison_against_torchs_float32_interpolate():
    peak = 0.0
    for k, ((H, W), (Ho, Wo)) in enumerate(SHAPES):
        img = np.random.RandomState(k).random_sample((3, H, W)).astype(np.float32)
        mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
        n = torch.from_numpy(O.transform_normalize(img, mean, std))
        got = F.interpolate(n[None], size=(Ho, Wo), mode="bilinear", align_corners=False).numpy()
        units = O.input_transform_compare(got, *O.input_transform64([img], [mean], [std], [(Ho, Wo)], Ho, Wo))
        print("torch CPU float32 %s -> %s: peak %.2f x 2^-24 M" % ((H, W), (Ho, Wo), units))
        peak = max(peak, units)
    assert 0.0 < peak <= O.TRANSFORM_BOUND


def test_restated_positions_pass_the_comparison_against_the_references_goldens():
    """tests/golden/net_transforms.npz: the reference's own transform on the CPU in float32 (oracle/gen_goldens.py)."""
    imgs, _, means, stds = GG.net_transform_inputs()
    imgs = [i.numpy() for i in imgs]
    default = ([[0.485, 0.456, 0.406]] * 2, [[0.229, 0.224, 0.225]] * 2)
    for tag, (m, s), crop in (("train", (means, stds), False), ("eval", default, False), ("crop", default, True)):
        want = G["nt_%s_batch" % tag]
        sizes = [tuple(int(v) for v in row) for row in G["nt_%s_sizes" % tag]]
        assert any(sz != i.shape[1:] for sz, i in zip(sizes, imgs))
        units = O.input_transform_compare(want, *O.input_transform64(imgs, m, s, sizes, want.shape[2], want.shape[3], crop))
        print("golden %s: peak %.2f x 2^-24 M" % (tag, units))
        assert units <= O.TRANSFORM_BOUND
    one = torch.rand(3, 64, 100, generator=torch.Generator().manual_seed(8)).numpy()
    want = G["nt_unit_batch"]
    O.input_transform_compare(want, *O.input_transform64([one], default[0][:1], default[1][:1], None, want.shape[2], want.shape[3]))


def test_quantise_restatement_equals_the_transforms_for_every_half_in_the_domain():
    from detectinblur_amd.models.net_transforms import GeneralizedRCNNTransform
    x = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    domain = torch.isfinite(x) & (x >= 0) & ((x.float() * 255).half() < 256)
    assert int(domain.sum()) == 15364 + 1                                       # +0 .. 0x3C03 (1.0029297), and -0
    x = x[domain]
    want = GeneralizedRCNNTransform.quantize(x)
    got = O.transform_quantize(x.numpy())
    assert got.dtype == np.float16 and np.array_equal(got.view(np.uint16), want.numpy().view(np.uint16))
    with pytest.raises(ValueError):
        O.transform_quantize(np.array([1.01], dtype=np.float16))
    vals = quantise_domain_values()
    assert vals.max() == np.float16(1.0029297) and set(O.transform_quantize(vals).view(np.uint16)) == set(
        (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float16).view(np.uint16))
