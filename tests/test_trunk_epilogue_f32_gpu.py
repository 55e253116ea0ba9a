"""The fp32 half of the trunk's epilogue family (csrc/dib_eltwise_vec.h at 4 fp32 per lane, the scalar and the transposing kernel
of csrc/dib_eltwise.hip) called straight through the C ABI, the way tests/test_amp_gpu.py calls the bf16 half: random inputs
salted with NaN, +-inf, +-0, denormals, against the host references of oracle/dib_oracle.py A21 (numpy; held to torch on the CPU
by tests/test_trunk_epilogue_reference.py) bit for bit, NaN by position; every call twice.  The stem pool also through its bf16
entries.  What this pins beyond the autograd-level tests of tests/test_detector_ops.py: every fused ReLU lets a NaN through
(torch's relu does; a bare fmaxf(v, 0) returns 0), the stem pool selects a NaN as ATen's max_pool2d does (a NaN beats
everything, the last NaN of a window is the recorded one), cleared elements are +0, a NaN carries no mask bit, elements off the
strided grid of the scatter are untouched.  At the end the same property through the modules: a NaN pixel of the input image
reaches every pyramid level of its image and no level of the other."""
import numpy as np
import pytest
import torch

import dib_oracle as O
from tests.test_trunk_epilogue_reference import (SCALAR_SHAPE, SCATTER_CASES, SHAPES, STEM_SHAPES, TOPDOWN_CASES, TRANSPOSE_SHAPES, rand_bias,
                                                 rand_nhwc, same_bits, stem_input)

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _lib():
    from detectinblur_amd import _lib as L
    return L


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _twice(call, *inputs):
    """call(*fresh device copies of inputs) -> device tensors; run twice, the two results bitwise equal; returns the first as numpy"""
    outs = []
    for _ in range(2):
        res = call(*[_dev(a) if a is not None else None for a in inputs])
        outs.append([_host(t) for t in (res if isinstance(res, (tuple, list)) else (res,))])
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes(), "two calls on the same input differ"
    return outs[0] if len(outs[0]) > 1 else outs[0][0]


def test_bias_act_f32_kernels_bit_for_bit():
    L = _lib()
    l = L.lib()
    for k, shape in enumerate(SHAPES + [SCALAR_SHAPE]):
        C = shape[1]
        x0, r0, bias = rand_nhwc(shape, 10 + k), rand_nhwc(shape, 50 + k, roll=1), rand_bias(C, k)
        b = _dev(bias)
        for res in (False, True):
            for relu in (False, True):
                want = O.bias_act32(x0, bias, r0 if res else None, relu)

                def plain(x, r):
                    L.check(l.dib_bias_act_nhwc(x.data_ptr(), b.data_ptr(), r.data_ptr() if res else None, x.numel(), C, int(relu), L.stream_of(x)))
                    return x

                got = _twice(plain, x0, r0 if res else None)
                assert same_bits(got, want), (shape, res, relu, int(np.isnan(got).sum()), int(np.isnan(want).sum()))
                if relu and x0.size > 4:         # every shape but the single pixel (vector and scalar kernel) carries a NaN through
                    assert np.isnan(want).any(), (shape, res)        # its ReLU; with a residual, one born in the kernel (inf - inf)
                    assert not res or (np.isnan(want) & ~np.isnan(x0) & ~np.isnan(r0)).any(), (shape, res)
                if relu and C % 4 == 0:
                    def masked(x, r):
                        mask = torch.full((x.numel() // 4,), 0xAA, dtype=torch.uint8, device="cuda")
                        L.check(l.dib_bias_act_mask_nhwc(x.data_ptr(), b.data_ptr(), r.data_ptr() if res else None, x.numel(), C, mask.data_ptr(),
                                                         L.stream_of(x)))
                        return x, mask

                    got, mask = _twice(masked, x0, r0 if res else None)
                    assert same_bits(got, want), (shape, res, "mask form")
                    assert np.array_equal(mask, O.sign_mask(want)), (shape, res)           # bytes; a NaN carries no bit
        # in-place aliasing: the residual IS the tensor (x = act((x + bias) + x))
        x = _dev(x0)
        L.check(l.dib_bias_act_nhwc(x.data_ptr(), b.data_ptr(), x.data_ptr(), x.numel(), C, 1, L.stream_of(x)))
        assert same_bits(_host(x), O.bias_act32(x0, bias, x0, True)), shape
    torch.cuda.synchronize()


def test_bias_act_transpose_bit_for_bit():
    L = _lib()
    l = L.lib()
    for k, shape in enumerate(TRANSPOSE_SHAPES):
        N, C, H, W = shape
        x0, bias = rand_nhwc(shape, 15 + k), rand_bias(C, 3 + k)
        b = _dev(bias)
        for to_planar in (1, 0):
            for relu in (0, 1):
                y = O.bias_act32(x0, bias, None, bool(relu))
                assert np.isnan(y).any() and np.isinf(y).any(), shape          # through the ReLU too
                src = x0 if to_planar else np.ascontiguousarray(x0.transpose(0, 3, 1, 2))
                want = np.ascontiguousarray(y.transpose(0, 3, 1, 2)) if to_planar else y

                def call(x):
                    out = torch.full(want.shape, 7.0, device="cuda")
                    L.check(l.dib_bias_act_transpose(x.data_ptr(), b.data_ptr(), out.data_ptr(), N, C, H * W, to_planar, relu, L.stream_of(x)))
                    return out

                assert same_bits(_twice(call, src), want), (shape, to_planar, relu)
    torch.cuda.synchronize()


def test_relu_mask_backward_and_add_relu_mask_f32_bit_for_bit():
    L = _lib()
    l = L.lib()
    for k, shape in enumerate(SHAPES):
        g0, b0 = rand_nhwc(shape, 20 + k), rand_nhwc(shape, 30 + k, roll=1)
        mask0 = np.random.RandomState(k).randint(0, 16, g0.size // 4).astype(np.uint8)
        keep = O.mask_bits(mask0).reshape(g0.shape)
        mask = _dev(mask0)
        want = O.mask_select(g0, mask0)

        def bwd(g):
            out = torch.full_like(g, 7.0)
            L.check(l.dib_relu_mask_backward(g.data_ptr(), mask.data_ptr(), out.data_ptr(), g.numel(), L.stream_of(g)))
            return out

        got = _twice(bwd, g0)
        assert same_bits(got, want), shape
        assert not got.view(np.uint32)[~keep].any()                                       # cleared elements are +0 in bits
        alias = _dev(g0)
        L.check(l.dib_relu_mask_backward(alias.data_ptr(), mask.data_ptr(), alias.data_ptr(), alias.numel(), L.stream_of(alias)))   # in place
        assert _host(alias).tobytes() == got.tobytes()
        for m in (None, mask0):
            def add(a, b):
                L.check(l.dib_add_relu_mask(a.data_ptr(), b.data_ptr(), mask.data_ptr() if m is not None else None, a.numel(), L.stream_of(a)))
                return a

            got = _twice(add, g0, b0)
            assert same_bits(got, O.add_relu_mask32(g0, b0, m)), (shape, m is None)
            if m is not None:
                assert not got.view(np.uint32)[~keep].any()
        # a = a + a: both operands the same tensor
        a = _dev(g0)
        L.check(l.dib_add_relu_mask(a.data_ptr(), a.data_ptr(), mask.data_ptr(), a.numel(), L.stream_of(a)))
        assert same_bits(_host(a), O.add_relu_mask32(g0, g0, mask0)), shape
    torch.cuda.synchronize()


def test_scatter_add_f32_bit_for_bit_and_nothing_off_the_grid_moves():
    L = _lib()
    l = L.lib()
    for k, (N, C, H, W, s) in enumerate(SCATTER_CASES):
        Hs, Ws = (H - 1) // s + 1, (W - 1) // s + 1
        a0, b0 = rand_nhwc((N, C, H, W), 40 + k), rand_nhwc((N, C, Hs, Ws), 60 + k, roll=1)

        def call(a, b):
            L.check(l.dib_scatter_add_nhwc(a.data_ptr(), b.data_ptr(), N, H, W, Hs, Ws, C, s, L.stream_of(a)))
            return a

        got = _twice(call, a0, b0)
        assert same_bits(got, O.scatter_add32(a0, b0, s)), (N, C, H, W, s)
        off = np.ones((H, W), dtype=bool)
        off[::s, ::s] = False
        assert got[:, off].tobytes() == a0[:, off].tobytes()                               # NaN payloads included
    torch.cuda.synchronize()


def test_fpn_topdown_merge_f32_against_the_host_reference():
    L = _lib()
    l = L.lib()
    for k, (N, C, H, W, Ht, Wt) in enumerate(TOPDOWN_CASES):
        x0, top0, bias = rand_nhwc((N, C, H, W), 70 + k), rand_nhwc((N, C, Ht, Wt), 80 + k, roll=1), rand_bias(C, 7 + k)
        b = _dev(bias)

        def call(x, top):
            L.check(l.dib_fpn_topdown_merge_nhwc(x.data_ptr(), b.data_ptr(), top.data_ptr(), N, H, W, Ht, Wt, C, L.stream_of(x)))
            return x

        assert same_bits(_twice(call, x0, top0), O.topdown_merge32(x0, bias, top0)), (N, C, H, W)
    torch.cuda.synchronize()


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_stem_pool_selects_and_keeps_nan_like_max_pool2d(bf16):
    """pooled values bit for bit (bf16: the fp32 values rounded once), `arg` exactly -- NaN windows included: the last NaN in
    row-major window order --, the dense gradient at the tolerance of test_stem_bias_relu_maxpool_in_one_pass_equals_the_three_torch_ops
    (up to four windows are summed in fp32) against the float64 scatter."""
    L = _lib()
    l = L.lib()
    fwd = l.dib_stem_pool_forward_bf16 if bf16 else l.dib_stem_pool_forward
    bwd = l.dib_stem_pool_backward_bf16 if bf16 else l.dib_stem_pool_backward
    for k, shape in enumerate(STEM_SHAPES):
        N, C, H, W = shape
        x0, bias = stem_input(shape, k)
        b = _dev(bias)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        pooled, pos = O.stem_pool32(x0, bias)
        want_arg = O.pack_pool_arg(pos)

        def forward(x):
            out = torch.full((N, Ho, Wo, C), 7.0, device="cuda", dtype=torch.bfloat16 if bf16 else torch.float32)
            arg = torch.full((N * Ho * Wo * (C // 4),), -1, dtype=torch.int16, device="cuda")
            L.check(fwd(x.data_ptr(), b.data_ptr(), out.data_ptr(), arg.data_ptr(), N, H, W, C, L.stream_of(x)))
            return (out.view(torch.int16) if bf16 else out), arg

        out, arg = _twice(forward, x0)
        if bf16:
            assert same_bits(O.from_bf16_bits(out.view(np.uint16)), O.from_bf16_bits(O.to_bf16_bits(pooled))), shape
        else:
            assert same_bits(out, pooled), (shape, int(np.isnan(out).sum()), int(np.isnan(pooled).sum()))
        assert np.array_equal(arg.view(np.uint16), want_arg), shape
        g0 = np.random.RandomState(100 + k).standard_normal((N, Ho, Wo, C)).astype(np.float32)
        if bf16:
            g0 = O.from_bf16_bits(O.to_bf16_bits(g0))
        want_g = O.stem_pool_backward64(g0, pos, H, W)
        arg_dev = _dev(want_arg.view(np.int16))

        def backward(g):
            gx = torch.full((N, H, W, C), 7.0, device="cuda")
            gg = g.to(torch.bfloat16) if bf16 else g
            L.check(bwd(gg.data_ptr(), arg_dev.data_ptr(), gx.data_ptr(), N, H, W, C, L.stream_of(g)))
            return gx

        gx = _twice(backward, g0)
        assert np.allclose(gx.astype(np.float64), want_g, rtol=1e-6, atol=1e-6), (shape, float(np.abs(gx - want_g).max()))
    torch.cuda.synchronize()


# ---- through the modules ---------------------------------------------------------------------------------------------------------

def _nan_image():
    g = torch.Generator().manual_seed(4)
    img = torch.randn((2, 3, 64, 96), generator=g)
    img[1, :, 20, 30] = NAN
    return img.cuda().contiguous(memory_format=torch.channels_last)


def test_stem_keeps_a_nan_pixel_with_and_without_the_fused_pool():
    from detectinblur_amd.models import backbone as B
    from tests.test_amp_gpu import _randomize_bn
    torch.manual_seed(6)
    body = B.ResNet50Body().cuda().to(memory_format=torch.channels_last)
    _randomize_bn(body)
    img = _nan_image()
    old, family, taken = B.FUSE_STEM_POOL, B._lib.family, []
    assert old is True
    B._lib.family = lambda member, dtype: (taken.append(member), family(member, dtype))[1]
    try:
        with torch.no_grad():
            fused = B.stem(img, body.conv1, body.bn1)
            assert taken == ["stem_pool_forward"], taken                      # the fused pool ran
            B.FUSE_STEM_POOL = False
            plain = B.stem(img, body.conv1, body.bn1)
            assert "stem_pool_forward" not in taken[1:], taken
    finally:
        B.FUSE_STEM_POOL, B._lib.family = old, family
    fn, pn = torch.isnan(fused), torch.isnan(plain)
    assert bool(pn[1].any()) and not bool(pn[0].any())
    assert torch.equal(fn, pn), (int(fn.sum()), int(pn.sum()))
    assert torch.equal(torch.where(fn, torch.zeros_like(fused), fused), torch.where(pn, torch.zeros_like(plain), plain))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "amp"])
@pytest.mark.parametrize("grad", [False, True], ids=["inference", "training"])
def test_a_nan_pixel_reaches_every_pyramid_level_of_its_image_only(dtype, grad):
    """resnet_fpn_backbone with every fusion on: inference takes the transposing epilogues, training the mask forms and the entry
    nodes.  The reference's trunk (plain torch modules) propagates the NaN to the loss, where `Loss is nan` stops the run."""
    from detectinblur_amd.models import backbone as B
    from tests.test_amp_gpu import _randomize_bn
    torch.manual_seed(11)
    net = B.resnet_fpn_backbone("resnet50", False, trainable_layers=5).cuda().to(memory_format=torch.channels_last)
    _randomize_bn(net)
    net.compute_dtype = dtype
    img = _nan_image()
    with torch.set_grad_enabled(grad):
        out = net(img)
    assert len(out) == 5
    for k, v in out.items():
        v = v.detach().float()
        assert bool(torch.isnan(v[1]).any()), (k, "the NaN of image 1 was erased")
        assert bool(torch.isfinite(v[0]).all()), (k, "image 0 is not finite")
