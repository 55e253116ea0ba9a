"""The DeepDeblur trainer without a GPU: the draw order and the patch geometry against the reference's dataCommon.py (which imports
scikit-image and cannot be imported here: its order is restated below with line citations), the torch restatements of the two
reduction kernels against float64 definitions, their summation order restated in numpy float32 from the header of
csrc/dib_deblur_train.hip (against float64 sums and against the two depth helpers; tests/test_deblur_train_geometry_gpu.py holds the
kernels to it bit for bit), the torch path of the network, and the driver end to end on the CPU."""
import collections
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


# ---- THE SUMMATION ORDER, restated in numpy float32 -----------------------------------------------------------------------------
# Written from the header comment of csrc/dib_sliced_sum.h ("THE SUMMATION ORDER ... fixed by the shape alone"), not from the
# kernel bodies: tests/test_deblur_train_geometry_gpu.py holds the kernels to these bit for bit.  Both reductions have one structure:
# n items in memory order are cut into S slices of consecutive items; W lanes walk a slice, lane w adding items w, w + W, ... one
# after the other; the W lane sums are added as a tree; the S slice sums are added one after the other from slice 0.  `_walk` states
# that structure once, over an algebra: `_F32` carries the values (every addition rounds once), `_Depth` carries, instead of a value,
# the largest number of additions any one input has passed through on its way into it -- what DT.bias_grad_depth / DT.l1_loss_depth
# claim to be -- and needs no data, only the geometry.

BiasGradShape = collections.namedtuple("BiasGradShape", "V QB R chunks S L")


def _ceil_div(a, b):
    return -(-a // b)


def slice_begins(n, S):
    """begin of slice s = 0..S (S: the end): the first n % S slices are one item longer"""
    s = np.arange(S + 1, dtype=np.int64)
    return n // S * s + np.minimum(n % S, s)


def bias_grad_shape(n_pix, C, V):
    """(b) of the header: V channels per lane, QB = min(C / V, 256) lane columns and R = 256 / QB pixel rows per workgroup, `chunks`
    workgroups side by side, S = ceil(n_pix / (16 R)) slices capped at 1024, L = ceil(longest slice / R) additions per lane."""
    QB = min(C // V, 256)
    R = 256 // QB
    S = max(1, min(1024, _ceil_div(n_pix, 16 * R)))
    L = _ceil_div(int(np.diff(slice_begins(n_pix, S)).max()), R)
    return BiasGradShape(V, QB, R, _ceil_div(C // V, QB), S, L)


def l1_shape(n_pix):
    """(c) of the header: (S, L) of the 3 n_pix differences: S = ceil(3 n_pix / 2048) capped at 1024, L = ceil(longest slice / 256)"""
    S = max(1, min(1024, _ceil_div(3 * n_pix, 2048)))
    return S, _ceil_div(int(np.diff(slice_begins(3 * n_pix, S)).max()), 256)


class _F32:
    def __init__(self, items):
        self.items = np.ascontiguousarray(items, dtype=np.float32)             # [n, ...]

    def zero(self, S, W):
        return np.zeros((S, W) + self.items.shape[1:], dtype=np.float32)

    def chain(self, acc, idx, valid):
        x = self.items[np.minimum(idx, len(self.items) - 1)]
        x[~valid] = 0                               # a lane past its slice's end adds nothing; x + 0 == x bit for bit (no sum here is -0)
        return acc + x

    @staticmethod
    def add(a, b):
        return a + b


class _Depth:
    EMPTY = -(1 << 40)                              # a sum that no input has entered yet

    def zero(self, S, W):
        return np.full((S, W), self.EMPTY, dtype=np.int64)

    def chain(self, acc, idx, valid):
        return np.where(valid, np.maximum(acc, 0) + 1, acc)      # the item comes with no addition behind it

    @staticmethod
    def add(a, b):
        return np.maximum(a, b) + 1


def _walk(n, S, W, ops):
    begin = slice_begins(n, S)
    lanes = np.arange(W, dtype=np.int64)
    acc = ops.zero(S, W)
    for j in range(_ceil_div(int(np.diff(begin).max()), W)):     # the lane chain, in item order: w, w + W, w + 2 W, ...
        idx = begin[:-1, None] + lanes[None, :] + j * W
        acc = ops.chain(acc, idx, idx < begin[1:, None])
    h = 1
    while h < W:
        h *= 2
    h //= 2
    while h >= 1:                                   # the tree: row r takes row r + h, largest h first, only where r + h < W
        m = min(h, W - h)
        acc[:, :m] = ops.add(acc[:, :m], acc[:, h:h + m])
        h //= 2
    total = acc[0, 0]
    for s in range(1, S):                           # the slices, one after the other from slice 0
        total = ops.add(total, acc[s, 0])
    return total


def restated_bias_grad(values, V):
    """fp32 `values` [n_pix, C] (the masked gradient; Half values are exact in fp32) -> bias_grad [C] in the header's order"""
    n_pix, C = values.shape
    g = bias_grad_shape(n_pix, C, V)
    return _walk(n_pix, g.S, g.R, _F32(values))


def restated_bias_grad_depth(n_pix, C, V):
    g = bias_grad_shape(n_pix, C, V)
    return int(_walk(n_pix, g.S, g.R, _Depth()))


def restated_l1(out, target, stride, gscale, loss=0.0):
    """fp32 out [n_pix, 3], target [n_pix, stride] -> (the loss scalar after this level, the gradient [n_pix, 3]) in the header's
    order: out - target in fp32, fabsf, the chain with stride 256, eight tree levels, the slices from slice 0, one division by
    float(3 n_pix), one addition onto the scalar."""
    out = np.asarray(out, dtype=np.float32).reshape(-1, 3)
    n = out.size
    d = out - np.asarray(target, dtype=np.float32).reshape(-1, stride)[:, :3]
    total = _walk(n, l1_shape(n // 3)[0], 256, _F32(np.abs(d).reshape(-1)))
    denom = np.float32(n)
    k = np.float32(gscale) / denom
    grad = np.where(d != d, d, np.where(d > 0, k, np.where(d < 0, -k, np.float32(0)))).astype(np.float32)
    return np.float32(loss) + total / denom, grad


def restated_l1_depth(n_pix):
    return int(_walk(3 * n_pix, l1_shape(n_pix)[0], 256, _Depth()))


def _real_draw(rs, *shape):
    """the GPU tests' draw, randn * exp(6 rand): magnitudes spread over e^6, so that the order of the additions shows in the result"""
    return (rs.standard_normal(shape) * np.exp(6 * rs.random_sample(shape))).astype(np.float32)


# (n_pix, C, V): every V; R from 1 to 128 and 85 (no power of two); one and several slices, even and uneven; one and two chunks
SMALL_BIAS_GRAD = [(1, 64, 4), (5, 3, 1), (255, 12, 4), (257, 3, 1), (4099, 64, 4), (2049, 8, 4), (4099, 8, 4), (300, 8, 8),
                   (1000, 64, 8), (700, 64, 1), (37, 1028, 4), (5, 2056, 8), (4099, 12, 1)]
# ... and shapes at and past the 1024-slice cap, the trainer's own call last: for the depth alone, which needs no data
CAPPED_BIAS_GRAD = [(1392640, 3, 1), (1392641, 3, 1), (262144, 64, 4), (262145, 64, 4), (600001, 64, 4), (16385, 1024, 4),
                    (16391, 1028, 4), (524289, 64, 8), (16385, 2056, 8), (65537, 64, 1), (16 * 256 * 256, 64, 4)]
SMALL_L1 = [1, 7, 29, 683, 1027, 4099]
CAPPED_L1 = [170000, 699050, 699051, 1048576]


@pytest.mark.parametrize("n_pix,C,V", SMALL_BIAS_GRAD)
def test_restated_bias_grad_against_float64(n_pix, C, V):
    values = _real_draw(np.random.RandomState(1000 * C + n_pix), n_pix, C)
    got = restated_bias_grad(values, V)
    assert got.dtype == np.float32 and got.shape == (C,)
    v64 = values.astype(np.float64)
    bound = DT.bias_grad_depth(n_pix, C, V) * 2.0 ** -24 * np.abs(v64).sum(0)
    assert (np.abs(got.astype(np.float64) - v64.sum(0)) <= bound).all()


@pytest.mark.parametrize("n_pix", SMALL_L1)
def test_restated_l1_against_float64(n_pix):
    rs = np.random.RandomState(n_pix)
    out, target = _real_draw(rs, n_pix, 3), _real_draw(rs, n_pix, 6)
    target[0, 1] = out[0, 1]
    loss, grad = restated_l1(out, target, 6, 0.5, loss=3.0)
    assert loss.dtype == np.float32 and grad.dtype == np.float32
    d = out.astype(np.float64) - target[:, :3].astype(np.float64)
    want = np.abs(d).sum() / (3 * n_pix)
    # the subtraction, the tree, the division, the addition onto the scalar
    assert abs(float(loss) - (3.0 + want)) <= (DT.l1_loss_depth(n_pix) + 3) * 2.0 ** -24 * (3.0 + want)
    k = np.float32(0.5) / np.float32(3 * n_pix)
    assert np.array_equal(grad.astype(np.float64), np.sign(d) * float(k)) and grad[0, 1] == 0


@pytest.mark.parametrize("n_pix,C,V", SMALL_BIAS_GRAD + CAPPED_BIAS_GRAD)
def test_bias_grad_depth_is_the_restated_orders_longest_chain(n_pix, C, V):
    g = bias_grad_shape(n_pix, C, V)
    assert restated_bias_grad_depth(n_pix, C, V) == DT.bias_grad_depth(n_pix, C, V) == g.L + (g.R - 1).bit_length() + g.S - 1
    if (n_pix, C, V) in CAPPED_BIAS_GRAD:
        assert g.S == 1024 and n_pix >= 16 * g.R * 1024


@pytest.mark.parametrize("n_pix", SMALL_L1 + CAPPED_L1)
def test_l1_loss_depth_is_the_restated_orders_longest_chain(n_pix):
    S, L = l1_shape(n_pix)
    assert restated_l1_depth(n_pix) == DT.l1_loss_depth(n_pix) == L + 8 + S - 1
    assert (S == 1024) == (n_pix >= 699050)


def test_restated_order_is_not_any_order():
    """the restatement can tell the header's tree (largest h first) from the same additions smallest h first, on the GPU tests' draw"""
    values = _real_draw(np.random.RandomState(3), 4099, 8)
    g = bias_grad_shape(4099, 8, 4)
    assert (g.R, g.S) == (128, 3)
    lanes = _F32(values)
    acc = lanes.zero(g.S, g.R)
    begin = slice_begins(4099, g.S)
    for j in range(g.L):
        idx = begin[:-1, None] + np.arange(g.R)[None, :] + j * g.R
        acc = lanes.chain(acc, idx, idx < begin[1:, None])
    h = 1
    while h < g.R:                                  # smallest h first: still a sum of every lane, another order
        half = acc[:, ::2 * h].copy()
        half += acc[:, h::2 * h]
        acc[:, ::2 * h] = half
        h *= 2
    other = acc[0, 0] + acc[1, 0] + acc[2, 0]
    want = restated_bias_grad(values, 4)
    v64 = values.astype(np.float64)
    assert (np.abs(other.astype(np.float64) - v64.sum(0)) <= DT.bias_grad_depth(4099, 8) * 2.0 ** -24 * np.abs(v64).sum(0)).all()
    assert other.tobytes() != want.tobytes()


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
