"""The three kernel families of csrc/dib_deblur_train.hip at the trainer's launch geometry (-b 16 --patch_size 256, 64 features: a
million pixels, S = 1024 slices), where tests/test_deblur_train_gpu.py and tests/test_deblur_train_amp_gpu.py stay tiny.  The depth
bound of those files, depth * 2^-24 * sum |g|, is 6.5e-5 of sum |g| at that size and cannot see one lost pixel in a million, so the
sums here are held to two references that no summation order can blur, with no tolerance anywhere:

  (a) exact integers  small integer inputs: every partial sum is an integer below 2^24 (asserted from the int64 data), so every fp32
                      addition is exact in any order and the kernel's result must be the int64 sum, bit for bit.  A pixel lost or
                      counted twice at a slice seam moves the sum by a whole number.
  (b) the stated order  that file's header fixes the order of the additions by the shape alone; tests/test_deblur_train.py restates
                      it in numpy float32 (restated_bias_grad, restated_l1), and on real-valued inputs the kernels must give its
                      bits.  A kernel that sums correctly in another order fails here, and that is intended.

Each shape is the smallest that reaches its regime; the ids spell the regime out (R pixel rows per workgroup, S slices, L additions
per lane, channel chunks), computed from the header's rules by bias_grad_shape / l1_shape and asserted against the table the shapes
were chosen from.  Large inputs are drawn on the device; a case holds about 150 MB there (200 MB at 600,001 x 64, the largest)."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

from tests.test_deblur_train import TINY, bias_grad_shape, l1_shape, restated_bias_grad, restated_l1

pytestmark = pytest.mark.gpu

BLOCK = 1 << 16          # pixels per block where a tensor is filled or compared in blocks, to keep temporaries small
BOTH_FORMS_BYTES = 80 << 20


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _np_bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


# ---- (b) of the header: the bias gradient -------------------------------------------------------------------------------------------
# (C, n_pix, dtype, V, view) -> (R, S, L, chunks) it was chosen to reach.  `view`: the gradient lies one element into a larger buffer
# (2-byte aligned), which sends a Half gradient with C % 8 == 0 to the one-channel-per-lane form.
F32, F16 = torch.float32, torch.float16
BIAS_GRAD_ROWS = {
    (3, 1392640, F32, 1, False): (85, 1024, 16, 1),      # V = 1, 255 of 256 lanes active: S = 1024 exactly, uncapped
    (3, 1392641, F32, 1, False): (85, 1024, 17, 1),      # ... capped, with one longer slice
    (64, 262144, F32, 4, False): (16, 1024, 16, 1),      # the trainer's C at the cap boundary
    (64, 262145, F32, 4, False): (16, 1024, 17, 1),      # ... uneven slices, L 16 -> 17
    (64, 600001, F32, 4, False): (16, 1024, 37, 1),      # chains well past 16
    (1024, 16385, F32, 4, False): (1, 1024, 17, 1),      # QB = 256, R = 1: no LDS tree; capped
    (1028, 16391, F32, 4, False): (1, 1024, 17, 2),      # two channel chunks, the second with one active lane column
    (8, 2049, F32, 4, False): (128, 2, 9, 1),            # seven tree levels; the final kernel below one staging trip
    (8, 40000, F32, 4, False): (128, 20, 16, 1),
    (64, 70000, F32, 4, False): (16, 274, 16, 1),        # the final kernel's staging loop runs twice, uncapped
    (64, 524289, F16, 8, False): (32, 1024, 17, 1),      # Half, eight channels per lane, capped
    (2056, 16385, F16, 8, False): (1, 1024, 17, 2),      # ... two chunks, R = 1
    (64, 65537, F16, 1, True): (4, 1024, 17, 1),         # ... one channel per lane off sixteen bytes, capped
}


def _row_id(row):
    C, n_pix, dtype, V, view = row
    g = bias_grad_shape(n_pix, C, V)
    return "%s-C%d-n%d-V%d-R%d-S%d-L%d-chunks%d%s" % ("f16" if dtype == F16 else "f32", C, n_pix, V, g.R, g.S, g.L, g.chunks,
                                                    "-view" if view else "")


bias_grad_rows = pytest.mark.parametrize("row", list(BIAS_GRAD_ROWS), ids=_row_id)


def _check_row(row):
    """the regime the shape is for, and that the library's slice count is the restatement's"""
    from detectinblur_amd import _lib
    C, n_pix, dtype, V, view = row
    g = bias_grad_shape(n_pix, C, V)
    assert (g.R, g.S, g.L, g.chunks) == BIAS_GRAD_ROWS[row]
    if dtype == F32:
        assert V == (4 if C % 4 == 0 else 1) and _lib.lib().dib_bias_grad_workspace_bytes(n_pix, C) == g.S * C * 4
    else:
        # sized for the one-channel-per-lane form, whose slices are the shorter ones
        assert V == (8 if C % 8 == 0 and not view else 1)
        assert _lib.lib().dib_bias_grad_f16_workspace_bytes(n_pix, C) == bias_grad_shape(n_pix, C, 1).S * C * 4
    return g


def _place(row):
    """an uninitialised gradient [n_pix, C] of the row's dtype and alignment"""
    C, n_pix, dtype, V, view = row
    if not view:
        grad = torch.empty(n_pix, C, dtype=dtype, device="cuda")
        assert grad.data_ptr() % 16 == 0
        return grad
    buf = torch.empty(n_pix * C + 8, dtype=dtype, device="cuda")
    grad = buf[1:1 + n_pix * C].view(n_pix, C)
    assert grad.data_ptr() % 16 == 2
    return grad


def _relu_mask_backward(grad, mask):
    """the select the kernel must equal bit for bit: dib_relu_mask_backward for fp32; Half has no such entry point: +0 where the bit is
    clear, as tests/test_deblur_train_amp_gpu.py states it"""
    from detectinblur_amd import _lib
    from detectinblur_amd.models import deblur_train as DT
    if grad.dtype == F16:
        return DT.bias_grad_torch(grad, mask)[0]
    out = torch.empty_like(grad)
    _lib.check(_lib.lib().dib_relu_mask_backward(grad.data_ptr(), mask.data_ptr(), out.data_ptr(), grad.numel(), _lib.stream_of(grad)))
    return out


def _blocks(n_pix):
    return [(p0, min(n_pix, p0 + BLOCK)) for p0 in range(0, n_pix, BLOCK)]


def _assert_select(out, grad_in, mask, dtype):
    """out == the select of `grad_in` (any dtype holding the values) under `mask`, bit for bit, block by block"""
    n_pix, C = out.shape
    lane = 8 if dtype == F16 else 4
    for p0, p1 in _blocks(n_pix):
        want = _relu_mask_backward(grad_in[p0:p1].to(dtype), mask[p0 * C // lane:p1 * C // lane])
        assert torch.equal(_bits(out[p0:p1]), _bits(want)), p0


@bias_grad_rows
def test_bias_grad_exact_integers(row):
    """Reference (a): uniform integers in -3..3, plain and (where V > 1 allows a mask) masked, out of place and in place.  The masked
    gradient must be dib_relu_mask_backward's select bit for bit.  At 600,001 x 64 only the in-place form runs: a second gradient of
    154 MB would not fit the memory a case may take."""
    from detectinblur_amd.models import deblur_train as DT
    C, n_pix, dtype, V, view = row
    _check_row(row)
    g = _gen(7 * C + n_pix)
    src = torch.randint(-3, 4, (n_pix, C), generator=g, device="cuda", dtype=torch.int8)
    assert int(src.abs().sum(0, dtype=torch.int64).max()) < 2 ** 24           # every partial sum of a channel is exact in fp32
    exact = src.sum(0, dtype=torch.int64)
    if V > 1:
        y = torch.randint(-3, 4, (n_pix, C), generator=g, device="cuda", dtype=torch.int8)
        exact_masked = (src * (y > 0)).sum(0, dtype=torch.int64)
        assert int((exact_masked != exact).sum()) > 0
        mask = torch.cat([DT.sign_mask_torch(y[p0:p1].to(dtype)) for p0, p1 in _blocks(n_pix)])      # one byte per V elements
        assert mask.numel() == n_pix * C // V
        del y
    grad = _place(row)
    grad.copy_(src)
    same, bias = DT.bias_grad_device(grad)
    assert same is grad and bias.dtype == F32
    assert torch.equal(_bits(bias), _bits(exact.float()))
    if V == 1:
        return
    if grad.numel() * grad.element_size() <= BOTH_FORMS_BYTES:
        out, mbias = DT.bias_grad_device(grad, mask)
        assert out.data_ptr() != grad.data_ptr() and out.dtype == dtype
        assert torch.equal(_bits(mbias), _bits(exact_masked.float()))
        _assert_select(out, grad, mask, dtype)
        del out
    out, mbias = DT.bias_grad_device(grad, mask, out=grad)                    # in place
    assert out is grad and torch.equal(_bits(mbias), _bits(exact_masked.float()))
    _assert_select(grad, src, mask, dtype)


def _real_draw(row, seed):
    """the existing tests' draw, randn * exp(6 rand) (all finite in Half), filled in blocks"""
    C, n_pix, dtype, V, view = row
    g = _gen(seed)
    grad = _place(row)
    for p0, p1 in _blocks(n_pix):
        grad[p0:p1] = torch.randn(p1 - p0, C, generator=g, device="cuda") * torch.rand(p1 - p0, C, generator=g, device="cuda").mul_(6).exp_()
    return grad


@bias_grad_rows
def test_bias_grad_stated_order(row):
    """Reference (b) on a real-valued draw: the header's order, bit for bit (Half values are exact in fp32: one restatement serves
    fp32, Half V = 8 and Half V = 1); two runs give the same bits; a NaN in the last pixel of the last slice poisons channel C - 1 and
    leaves every other channel's bits; where the shape allows a mask, the masked sum in the same order."""
    from detectinblur_amd.models import deblur_train as DT
    C, n_pix, dtype, V, view = row
    _check_row(row)
    grad = _real_draw(row, 1000 * C + n_pix)
    assert torch.isfinite(grad).all()
    bias = DT.bias_grad_device(grad)[1]
    want = restated_bias_grad(grad.cpu().float().numpy(), V)
    assert np.array_equal(_np_bits(bias), want.view(np.int32))
    assert torch.equal(_bits(bias), _bits(DT.bias_grad_device(grad)[1]))
    if V > 1 and grad.numel() * grad.element_size() <= BOTH_FORMS_BYTES:
        g = _gen(n_pix)
        mask = torch.cat([DT.sign_mask_torch(torch.randn(p1 - p0, C, generator=g, device="cuda", dtype=dtype)) for p0, p1 in _blocks(n_pix)])
        out, mbias = DT.bias_grad_device(grad, mask)
        _assert_select(out, grad, mask, dtype)
        assert np.array_equal(_np_bits(mbias), restated_bias_grad(out.cpu().float().numpy(), V).view(np.int32))
        del out
    grad[n_pix - 1, C - 1] = float("nan")
    pb = DT.bias_grad_device(grad)[1]
    assert torch.isnan(pb[C - 1]) and torch.equal(_bits(pb[:C - 1]), _bits(bias[:C - 1]))


def test_bias_grad_workspace_is_sized_by_the_capped_slice_count():
    """ties the library's S to the restatement's and to the Python depth helper's at the cap"""
    from detectinblur_amd import _lib
    l = _lib.lib()
    assert l.dib_bias_grad_workspace_bytes(262144, 64) == 1024 * 64 * 4 and bias_grad_shape(262144, 64, 4).S == 1024
    assert l.dib_bias_grad_workspace_bytes(262145, 64) == 1024 * 64 * 4
    assert l.dib_bias_grad_workspace_bytes(262144 - 255, 64) == 1024 * 64 * 4 and l.dib_bias_grad_workspace_bytes(262144 - 256, 64) == 1023 * 64 * 4
    assert l.dib_bias_grad_workspace_bytes(1 << 30, 64) == 1024 * 64 * 4
    # the Half query is the one-channel-per-lane form's: R = 4 at C = 64, capped past 16 * 4 * 1024 pixels
    assert l.dib_bias_grad_f16_workspace_bytes(65536, 64) == 1024 * 64 * 4 and l.dib_bias_grad_f16_workspace_bytes(65537, 64) == 1024 * 64 * 4
    assert l.dib_bias_grad_f16_workspace_bytes(65536 - 64, 64) == 1023 * 64 * 4 and bias_grad_shape(65537, 64, 1).S == 1024


# ---- (c) of the header: the L1 loss ---------------------------------------------------------------------------------------------------
# n_pix -> (S, L): S = 1024 uncapped, capped with one longer chain, the trainer's level 0 (16 x 256 x 256), and a mid-size S
L1_ROWS = {699050: (1024, 8), 699051: (1024, 9), 1048576: (1024, 12), 170000: (250, 8)}
SENTINEL = -12345.0


def _l1_id(n_pix):
    return "n%d-S%d-L%d" % ((n_pix,) + l1_shape(n_pix))


l1_rows = pytest.mark.parametrize("n_pix", list(L1_ROWS), ids=_l1_id)
l1_strides = pytest.mark.parametrize("stride", [6, 3], ids=["stride6", "stride3"])


def _l1(out, target, gscale, loss):
    """the raw entry point into a gradient buffer filled with a sentinel, so that an element no lane visits shows"""
    from detectinblur_amd import _lib
    l = _lib.lib()
    n_pix = out.shape[0]
    assert l.dib_l1_pyramid_loss_workspace_bytes(n_pix) == l1_shape(n_pix)[0] * 4
    grad = torch.full_like(out, SENTINEL)
    work = torch.full((l1_shape(n_pix)[0],), float("nan"), device="cuda")
    _lib.check(l.dib_l1_pyramid_loss(out.data_ptr(), target.data_ptr(), int(target.shape[1]), n_pix, gscale, grad.data_ptr(), loss.data_ptr(),
                                     work.data_ptr(), _lib.stream_of(out)))
    return grad


@l1_strides
@l1_rows
def test_l1_exact_integers(n_pix, stride):
    """Reference (a): integer out and target with 1 <= |out - target| <= 4 everywhere but at a handful of planted zeros and negative
    zeros, so sum |d| is an integer below 2^24, exact in any order, and the loss is one division of it.

    The division: csrc/Makefile builds with -O3 -ffp-contract=off and with neither -ffast-math nor
    -fno-hip-fp32-correctly-rounded-divide-sqrt, so hipcc's default holds and the build's fp32 division is correctly rounded (the
    v_div_scale / v_div_fmas / v_div_fixup sequence).  The loss must therefore be numpy's float32(sum) / float32(3 n_pix), equal bits.
    One |d| >= 1 lost or counted twice moves the quotient by 1 / (3 n_pix) or more, which is above the spacing of fp32 there
    (asserted), so it cannot hide in the loss's last place."""
    assert l1_shape(n_pix) == L1_ROWS[n_pix]
    gscale = 0.5 if (n_pix, stride) == (170000, 3) else 1.0
    g = _gen(10 * n_pix + stride)
    t = torch.randint(-100, 101, (n_pix, stride), generator=g, device="cuda", dtype=torch.int32)
    d = torch.randint(1, 5, (n_pix, 3), generator=g, device="cuda", dtype=torch.int32) * (2 * torch.randint(0, 2, (n_pix, 3), generator=g, device="cuda", dtype=torch.int32) - 1)
    zeros = [(0, 0), (n_pix // 3, 1), (n_pix // 2, 2), (n_pix - 1, 2)]                # d == +0 ...
    neg_zeros = [(1, 1), (n_pix // 2 + 1, 0), (n_pix - 2, 1)]                        # ... and -0 - 0 == -0
    for p, c in zeros + neg_zeros:
        d[p, c] = 0
    for p, c in neg_zeros:
        t[p, c] = 0
    out, target = (t[:, :3] + d).float(), t.float()
    for p, c in neg_zeros:
        out[p, c] = -0.0
    total = int(d.abs().sum(dtype=torch.int64))
    assert total < 2 ** 24 and int((d == 0).sum()) == 7
    want = np.float32(total) / np.float32(3 * n_pix)
    assert np.spacing(want) * (3 * n_pix) < 1
    loss = torch.zeros(1, device="cuda")                                             # 0 + x: the addition onto the scalar is exact
    grad = _l1(out, target, gscale, loss)
    assert np.array_equal(_np_bits(loss), np.array([want]).view(np.int32)), (float(loss), want)
    k = np.float32(gscale) / np.float32(3 * n_pix)
    assert torch.equal(_bits(grad), _bits(torch.sign(d).float() * float(k)))         # +-k, +0 at either zero; no sentinel left
    # a second level onto the same scalar (the existing tests' 5 pixels): one more correctly rounded division and addition
    out2 = torch.tensor([[3.0, -1.0, 2.0]] * 5, device="cuda")
    _l1(out2, torch.zeros(5, 3, device="cuda"), 1.0, loss)
    assert np.array_equal(_np_bits(loss), np.array([want + np.float32(30) / np.float32(15)]).view(np.int32))


@l1_strides
@l1_rows
def test_l1_stated_order(n_pix, stride):
    """Reference (b) on real-valued inputs, onto a scalar that is not zero: the header's order down to the division (correctly
    rounded in this build: see test_l1_exact_integers) and the addition, equal bits; the gradient sign(d) * float32(gscale) /
    float32(3 n_pix) at every element; two runs give the same bits."""
    assert l1_shape(n_pix) == L1_ROWS[n_pix]
    gscale = 0.5 if (n_pix, stride) == (170000, 3) else 1.0
    g = _gen(10 * n_pix + stride + 1)
    out = torch.randn(n_pix, 3, generator=g, device="cuda") * torch.rand(n_pix, 3, generator=g, device="cuda").mul_(6).exp_()
    target = torch.randn(n_pix, stride, generator=g, device="cuda") * torch.rand(n_pix, stride, generator=g, device="cuda").mul_(6).exp_()
    target[n_pix // 2, 1] = out[n_pix // 2, 1]
    loss = torch.full((1,), 3.25, device="cuda")
    grad = _l1(out, target, gscale, loss)
    want_loss, want_grad = restated_l1(out.cpu().numpy(), target.cpu().numpy(), stride, gscale, loss=3.25)
    assert np.array_equal(_np_bits(loss), np.array([want_loss]).view(np.int32)), (float(loss), want_loss)
    assert np.array_equal(_np_bits(grad), want_grad.view(np.int32)) and float(grad[n_pix // 2, 1]) == 0
    again = torch.full((1,), 3.25, device="cuda")
    assert torch.equal(_bits(_l1(out, target, gscale, again)), _bits(grad)) and torch.equal(_bits(again), _bits(loss))


# ---- (a) of the header: patches -----------------------------------------------------------------------------------------------------

PATCH_SHAPES = [(3, 48, 56), (3, 51, 77), (3, 64, 59)]
ORDERS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


def _bit_patterns(shape, dtype, g):
    """every bit pattern, NaNs and denormals included: the kernel moves values and never converts them"""
    ibits = torch.int16 if dtype == F16 else torch.int32
    info = torch.iinfo(ibits)
    return torch.randint(info.min, info.max + 1, shape, generator=g, device="cuda", dtype=torch.int64).to(ibits).view(dtype)


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
@pytest.mark.parametrize("ps", [16, 17, 32, 40], ids=["ps16-1block", "ps17-2blocks-partial", "ps32-4blocks", "ps40-7blocks-partial"])
def test_patches_over_several_blocks(ps, dtype):
    """grid.x = ceil(ps^2 / 256) blocks per plane, where the existing tests have one: a full block, a full and a partial one, four
    full ones, six full and a partial one.  Patches at the origin, at the far corner and at two interior offsets with odd px, under all
    eight flips and transposes and all six channel orders, against torch indexing bit for bit."""
    from detectinblur_amd.models import deblur_train as DT
    assert -(-ps * ps // 256) == {16: 1, 17: 2, 32: 4, 40: 7}[ps] and (ps * ps % 256 != 0) == (ps in (17, 40))
    images = [_bit_patterns(s, dtype, _gen(5 + i)) for i, s in enumerate(PATCH_SHAPES)]
    corners = [lambda s: (0, 0), lambda s: (s[1] - ps, s[2] - ps), lambda s: (3, 5), lambda s: (s[1] - ps - 1, 11)]
    assert all(s[1] - ps >= 8 and s[2] - ps >= 16 for s in PATCH_SHAPES)
    for corner in corners:
        for bits in range(8):
            # one launch holds the three images under all six orders
            ims = [im for im in images for _ in ORDERS]
            draws = [DT.PatchDraw(*corner(s), bool(bits & 1), bool(bits & 2), bool(bits & 4), order) for s in PATCH_SHAPES for order in ORDERS]
            got = DT.gather_patches(ims, draws, ps)
            want = DT.gather_patches_torch(ims, draws, ps)
            assert got.shape == (18, 3, ps, ps) and got.dtype == dtype
            assert torch.equal(_bits(got), _bits(want)), (corner(PATCH_SHAPES[0]), bits)


def _many_patches(B, dtype):
    from detectinblur_amd.models import deblur_train as DT
    images = [_bit_patterns((3, 5 + b % 4, 6 + b % 3), dtype, _gen(b)) for b in range(B)]
    draws = [DT.PatchDraw(b % 2, (b // 2) % 3, bool(b & 1), bool(b & 2), bool(b & 4), ORDERS[b % 6]) for b in range(B)]
    return images, draws


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_patches_at_the_launch_limit_and_through_the_split(dtype):
    """64 images are one launch (blockIdx.z up to 63); 65 go through gather_patches' split into 64 + 1: image 64 must come out right
    and the second launch must leave images 0..63 as the first wrote them."""
    from detectinblur_amd.models import deblur_train as DT
    assert DT.PATCH_MAX_BATCH == 64
    images, draws = _many_patches(65, dtype)
    full = DT.gather_patches(images[:64], draws[:64], 4)
    assert torch.equal(_bits(full), _bits(DT.gather_patches_torch(images[:64], draws[:64], 4)))
    split = DT.gather_patches(images, draws, 4)
    assert split.shape == (65, 3, 4, 4)
    assert torch.equal(_bits(split[:64]), _bits(full))
    assert torch.equal(_bits(split[64]), _bits(DT.gather_patches_torch(images[64:], draws[64:], 4)[0]))


def test_patches_raw_entry_point_refuses_65_images():
    from detectinblur_amd import _lib
    from detectinblur_amd.models import deblur_train as DT
    import ctypes
    l = _lib.lib()
    images, draws = _many_patches(65, F32)
    out = torch.full((65, 3, 4, 4), SENTINEL, device="cuda")

    def run(B):
        return l.dib_deblur_patches(_lib.ptr_array([im.data_ptr() for im in images[:B]]), _lib.DIB_F32,
                                    _lib.int_array([int(im.shape[1]) for im in images[:B]]), _lib.int_array([int(im.shape[2]) for im in images[:B]]),
                                    _lib.int_array([d.py for d in draws[:B]]), _lib.int_array([d.px for d in draws[:B]]),
                                    (ctypes.c_uint * B)(*[DT.flags_word(d) for d in draws[:B]]), B, 4, out.data_ptr(), _lib.stream_of(out))

    assert run(65) == _lib.DIB_EINVAL and b"B <= 64" in l.dib_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and l.dib_device_status(0) == 0           # nothing was launched
    assert run(64) == 0
    assert bool((out[64] == SENTINEL).all()) and torch.equal(_bits(out[:64]), _bits(DT.gather_patches_torch(images[:64], draws[:64], 4)))


# ---- the driver: a multi-block patch launch issued by the trainer itself ----------------------------------------------------------------

def _drive(out_dir, *extra):
    from detectinblur_amd import train_deblurrer as TD
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        TD.main(["--synthetic", "--synthetic_images", "6", "--synthetic_size", "72", "88", "--device", "cuda", "-j", "0", "-b", "2",
                 "--patch_size", "32", "--print_freq", "1", "--epochs", "1", "--early_stop", "2", "--param_index", "1",
                 "--output_dir", str(out_dir)] + TINY + list(extra))
    return buf.getvalue()


def test_driver_trains_on_the_gpu_with_patches_of_four_blocks(tmp_path):
    """test_driver_trains_on_the_gpu_into_the_inference_stage with --patch_size 32: grid.x = 4 in the trainer's own patch launch"""
    from detectinblur_amd import _lib
    from detectinblur_amd.models import deblur
    from detectinblur_amd.models import deblur_train as DT
    saved = DT.FUSE_DEBLUR_TRAIN
    try:
        DT.FUSE_DEBLUR_TRAIN = True
        text = _drive(tmp_path)
    finally:
        DT.FUSE_DEBLUR_TRAIN = saved
    losses = [float(v) for v in re.findall(r"loss: ([0-9.einfa+-]+)", text)]
    assert len(losses) == 3 and all(np.isfinite(losses)), text[-2000:]
    assert text.count("path: hip") == 3 and "3 steps, 6 images, 0 left out" in text
    with contextlib.redirect_stdout(io.StringIO()):
        d = deblur.Deblurer(str(tmp_path), device="cuda")
    out = d.deblur_(torch.rand(3, 20, 28, device="cuda"))
    assert d.last_path == "hip" and out.shape == (3, 20, 28) and torch.isfinite(out).all()
    torch.cuda.synchronize()
    assert _lib.lib().dib_device_status(0) == 0


def test_amp_driver_trains_on_the_gpu_with_patches_of_four_blocks(tmp_path):
    """... and test_amp_driver_trains_on_the_gpu_into_the_inference_stage's first run likewise, under --amp"""
    from detectinblur_amd import _lib
    from detectinblur_amd.models import deblur
    from detectinblur_amd.models import deblur_train as DT
    saved = DT.FUSE_DEBLUR_TRAIN, DT.FUSE_DEBLUR_TRAIN_AMP
    try:
        DT.FUSE_DEBLUR_TRAIN = DT.FUSE_DEBLUR_TRAIN_AMP = True
        text = _drive(tmp_path, "--amp")
    finally:
        DT.FUSE_DEBLUR_TRAIN, DT.FUSE_DEBLUR_TRAIN_AMP = saved
    losses = [float(v) for v in re.findall(r"loss: ([0-9.einfa+-]+)", text)]
    assert len(losses) == 3 and all(np.isfinite(losses)), text[-2000:]
    assert text.count("path: hip-amp") == 3 and len(re.findall(r"scale: [0-9.e+]+", text)) == 3 and "3 steps, 6 images, 0 left out" in text
    with contextlib.redirect_stdout(io.StringIO()):
        d = deblur.Deblurer(str(tmp_path), device="cuda")
    out = d.deblur_(torch.rand(3, 20, 28, device="cuda"))
    assert d.last_path == "hip" and out.shape == (3, 20, 28) and torch.isfinite(out).all()
    torch.cuda.synchronize()
    assert _lib.lib().dib_device_status(0) == 0
