"""`--amp` on the GPU: every bf16 epilogue kernel bit for bit against the torch expression evaluated in fp32 and cast once,
the fused autograd nodes on bf16 against the plain-torch bf16 graph, the accuracy of the mode against stock autocast (measured
in the same run), graphed inference, and the two drivers."""
import contextlib
import io
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F = torch.nn.functional
BF = torch.bfloat16
CL = torch.channels_last
INF, NAN = float("inf"), float("nan")
# exact ties of the rounding (1 + 2^-8 lies halfway between two bf16 values: to even, down; 1 + 2^-7 + 2^-8: to even, up), both
# zeros, bf16's smallest denormal, +-inf, NaN
SPECIALS = [INF, -INF, NAN, 0.0, -0.0, 2.0 ** -133, -2.0 ** -133, 1.0, 1.0 + 2.0 ** -7, 2.0 ** -8, -2.0 ** -8, 3.0e38, -3.0e38]


def _lib():
    from detectinblur_amd import _lib as L
    return L


def _bits(t):
    return t.contiguous(memory_format=CL).view(torch.int16) if t.dim() == 4 else t.contiguous().view(torch.int16)


def _same(got, want):
    """bit for bit; NaN by position, not by payload"""
    assert got.dtype == want.dtype and got.shape == want.shape
    gn, wn = torch.isnan(got), torch.isnan(want)
    if not torch.equal(gn, wn):
        return False
    if got.dtype == BF:
        return bool(torch.equal(torch.where(gn, torch.zeros_like(got), got).view(torch.int16),
                                torch.where(wn, torch.zeros_like(want), want).view(torch.int16)))
    return bool(torch.equal(torch.where(gn, torch.zeros_like(got), got), torch.where(wn, torch.zeros_like(want), want)))


def _rand(shape, seed, specials=True, scale=1.0):
    """a channels-last bf16 tensor on the bf16 grid (sums of two land on exact ties often), with the special values spread over
    the first channels of a few pixels"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = (torch.randn(shape, device="cuda", generator=g) * scale).to(BF).contiguous(memory_format=CL)
    if specials:
        flat = t.permute(0, 2, 3, 1).reshape(-1)                  # a view: NHWC element order
        assert flat.data_ptr() == t.data_ptr()
        C = shape[1]
        vals = torch.tensor(SPECIALS, device="cuda").to(BF)
        for c in range(min(4, C)):                                 # every special meets bias channels 0..3 (0, -0, a denormal, random)
            idx = (torch.arange(len(SPECIALS), device="cuda") * 3 + seed % 5) * C + c
            idx = idx[idx < flat.numel()]
            flat[idx] = vals[:len(idx)]
    return t


def _bias(C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    b = torch.randn(C, device="cuda", generator=g)
    b[0], b[1] = 0.0, -0.0
    if C > 2:
        b[2] = 1e-45                                                # x = 0: a positive fp32 sum that is stored as zero
    return b


def _pack_mask(y):
    """one byte per 8 consecutive NHWC elements, bit k = element > 0"""
    bits = (y.permute(0, 2, 3, 1).reshape(-1, 8) > 0).to(torch.int32)
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], device=y.device, dtype=torch.int32)
    return (bits * w).sum(1).to(torch.uint8)


def _unpack_mask(mask, shape):
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], device=mask.device, dtype=torch.int32)
    bits = (mask.to(torch.int32)[:, None] & w) != 0
    N, C, H, W = shape
    return bits.reshape(N, H, W, C).permute(0, 3, 1, 2)


# the trunk's activation shapes at b = 1 (800 x 1344: layer1 / layer2 / layer4 outputs, an FPN level) and ragged toy shapes
SHAPES = [(1, 256, 200, 336), (1, 512, 100, 168), (1, 2048, 25, 42), (1, 64, 200, 336), (3, 8, 5, 7), (2, 64, 37, 53)]


def test_bias_act_bf16_kernels_bit_for_bit():
    L = _lib()
    l = L.lib()
    for k, shape in enumerate(SHAPES):
        C = shape[1]
        for res in (False, True):
            for relu in (False, True):
                x0, r, bias = _rand(shape, 10 + k), (_rand(shape, 50 + k) if res else None), _bias(C, k)
                v = x0.float() + bias.reshape(1, -1, 1, 1)
                if res:
                    v = v + r.float()
                want = (torch.relu(v) if relu else v).to(BF)
                outs = []
                for _ in range(2):                                   # two calls on the same input are equal
                    x = x0.clone(memory_format=torch.preserve_format)
                    L.check(l.dib_bias_act_bf16_nhwc(x.data_ptr(), bias.data_ptr(), r.data_ptr() if res else None, x.numel(), C, int(relu),
                                                     L.stream_of(x)))
                    outs.append(x)
                assert _same(outs[0], want), (shape, res, relu)
                assert torch.equal(_bits(outs[0]), _bits(outs[1]))
                if relu:
                    x = x0.clone(memory_format=torch.preserve_format)
                    mask = torch.full((x.numel() // 8,), 0xAA, dtype=torch.uint8, device="cuda")
                    L.check(l.dib_bias_act_mask_bf16_nhwc(x.data_ptr(), bias.data_ptr(), r.data_ptr() if res else None, x.numel(), C,
                                                          mask.data_ptr(), L.stream_of(x)))
                    assert _same(x, want), (shape, res)
                    assert torch.equal(mask, _pack_mask(want)), (shape, res)       # the STORED value > 0, as bytes
                    # a positive fp32 sum stored as zero carries no mask bit
                    tiny = (torch.relu(v) > 0) & (want == 0)
                    assert not bool((_unpack_mask(mask, shape) & tiny).any())
            # in-place aliasing: the residual IS the tensor (x = act(x + bias + x))
            x = _rand(shape, 90 + k)
            want = torch.relu(x.float() + bias.reshape(1, -1, 1, 1) + x.float()).to(BF)
            L.check(l.dib_bias_act_bf16_nhwc(x.data_ptr(), bias.data_ptr(), x.data_ptr(), x.numel(), C, 1, L.stream_of(x)))
            assert _same(x, want), shape
    torch.cuda.synchronize()


def test_relu_mask_backward_and_add_relu_mask_bf16_bit_for_bit():
    L = _lib()
    l = L.lib()
    for k, shape in enumerate(SHAPES):
        g, b = _rand(shape, 20 + k), _rand(shape, 30 + k)
        gen = torch.Generator(device="cuda").manual_seed(k)
        mask = torch.randint(0, 256, (g.numel() // 8,), device="cuda", dtype=torch.uint8, generator=gen)
        keep = _unpack_mask(mask, shape)
        want = torch.where(keep, g, torch.zeros_like(g))
        out = torch.empty_like(g)
        L.check(l.dib_relu_mask_backward_bf16(g.data_ptr(), mask.data_ptr(), out.data_ptr(), g.numel(), L.stream_of(g)))
        assert _same(out, want), shape
        assert not bool((out.view(torch.int16)[~keep] != 0).any())              # cleared elements are +0
        alias = g.clone(memory_format=torch.preserve_format)
        L.check(l.dib_relu_mask_backward_bf16(alias.data_ptr(), mask.data_ptr(), alias.data_ptr(), g.numel(), L.stream_of(g)))   # in place
        assert torch.equal(_bits(alias), _bits(out))
        s = (g.float() + b.float()).to(BF)
        for m in (None, mask):
            want = s if m is None else torch.where(keep, s, torch.zeros_like(s))
            outs = []
            for _ in range(2):
                a = g.clone(memory_format=torch.preserve_format)
                L.check(l.dib_add_relu_mask_bf16(a.data_ptr(), b.data_ptr(), m.data_ptr() if m is not None else None, a.numel(), L.stream_of(a)))
                outs.append(a)
            assert _same(outs[0], want), (shape, m is None)
            assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    # the ties really occur: sums that lie exactly halfway between two bf16 values
    a, b = torch.tensor([1.0, 1.0 + 2.0 ** -7] * 4, device="cuda").to(BF), torch.tensor([2.0 ** -8] * 8, device="cuda").to(BF)
    L.check(l.dib_add_relu_mask_bf16(a.data_ptr(), b.data_ptr(), None, 8, L.stream_of(a)))
    assert a.float().tolist() == [1.0, 1.0 + 2.0 ** -6] * 4
    torch.cuda.synchronize()


def test_scatter_add_and_topdown_merge_bf16_bit_for_bit():
    L = _lib()
    l = L.lib()
    # a: conv1's data gradient, b: the strided convolution's on the gathered pixels (even and odd sizes)
    for k, (N, C, H, W, s) in enumerate(((1, 256, 200, 336, 2), (1, 1024, 50, 84, 2), (2, 64, 37, 53, 2), (3, 8, 5, 7, 2), (2, 16, 9, 6, 3))):
        Hs, Ws = (H - 1) // s + 1, (W - 1) // s + 1
        a0, b = _rand((N, C, H, W), 40 + k), _rand((N, C, Hs, Ws), 60 + k)
        want = a0.clone(memory_format=torch.preserve_format)
        want[:, :, ::s, ::s] = (a0[:, :, ::s, ::s].float() + b.float()).to(BF)
        outs = []
        for _ in range(2):
            a = a0.clone(memory_format=torch.preserve_format)
            L.check(l.dib_scatter_add_bf16_nhwc(a.data_ptr(), b.data_ptr(), N, H, W, Hs, Ws, C, s, L.stream_of(a)))
            outs.append(a)
        assert _same(outs[0], want), (N, C, H, W)
        assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    for k, (N, C, H, W, Ht, Wt) in enumerate(((1, 256, 200, 336, 100, 168), (8, 256, 50, 84, 25, 42), (2, 256, 51, 101, 26, 51), (1, 64, 7, 9, 4, 5),
                                              (3, 8, 33, 20, 11, 7))):
        x0, top, bias = _rand((N, C, H, W), 70 + k), _rand((N, C, Ht, Wt), 80 + k), _bias(C, 7 + k)
        want = ((x0.float() + bias.reshape(1, -1, 1, 1)) + F.interpolate(top.float(), size=(H, W), mode="nearest")).to(BF)
        outs = []
        for _ in range(2):
            x = x0.clone(memory_format=torch.preserve_format)
            L.check(l.dib_fpn_topdown_merge_bf16_nhwc(x.data_ptr(), bias.data_ptr(), top.data_ptr(), N, H, W, Ht, Wt, C, L.stream_of(x)))
            outs.append(x)
        assert _same(outs[0], want), (N, C, H, W)
        assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    torch.cuda.synchronize()


def test_stem_pool_bf16_follows_the_fp32_kernel():
    """fp32 convolution output in, bf16 pooled tensor out: the pooled values are the torch ops' rounded once, `arg` is the fp32
    kernel's (same window order and tie rule: inputs on the bf16 grid make ties common), and the backward pass on a bf16
    gradient equals the fp32 kernel's on the same gradient upcast."""
    L = _lib()
    l = L.lib()
    for k, (N, C, H, W) in enumerate(((1, 64, 400, 672), (2, 64, 40, 56), (1, 64, 37, 51), (3, 8, 9, 12), (1, 4, 1, 1), (1, 4, 2, 5))):
        g = torch.Generator(device="cuda").manual_seed(k)
        x = torch.randn((N, C, H, W), device="cuda", generator=g).to(BF).float().contiguous(memory_format=CL)      # ties
        if H > 2 and W > 2:
            x[:, :, 1::3, 1::4] = x[:, :, 0::3, 0::4][:, :, :x[:, :, 1::3, 1::4].shape[2], :x[:, :, 1::3, 1::4].shape[3]]
            x[0, :, 0, 0] = INF
            x[0, :, 2, 2] = -INF
        bias = torch.randn(C, device="cuda", generator=g).to(BF).float()
        bias[0] = 0.0
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        want = F.max_pool2d(torch.relu(x + bias.reshape(1, -1, 1, 1)), 3, stride=2, padding=1).to(BF)
        out32 = torch.empty((N, C, Ho, Wo), device="cuda").contiguous(memory_format=CL)
        arg32 = torch.empty((N * Ho * Wo * (C // 4),), dtype=torch.int16, device="cuda")
        L.check(l.dib_stem_pool_forward(x.data_ptr(), bias.data_ptr(), out32.data_ptr(), arg32.data_ptr(), N, H, W, C, L.stream_of(x)))
        outs = []
        for _ in range(2):
            out = torch.empty((N, C, Ho, Wo), device="cuda", dtype=BF).contiguous(memory_format=CL)
            arg = torch.empty_like(arg32)
            L.check(l.dib_stem_pool_forward_bf16(x.data_ptr(), bias.data_ptr(), out.data_ptr(), arg.data_ptr(), N, H, W, C, L.stream_of(x)))
            outs.append((out, arg))
        assert _same(outs[0][0], want), (N, C, H, W)
        assert torch.equal(outs[0][0].view(torch.int16), out32.to(BF).view(torch.int16))
        assert torch.equal(outs[0][1], arg32) and torch.equal(outs[1][1], arg32)
        assert torch.equal(outs[0][0].view(torch.int16), outs[1][0].view(torch.int16))
        go = torch.randn((N, C, Ho, Wo), device="cuda", generator=g).to(BF).contiguous(memory_format=CL)
        go32 = go.float()
        gx32 = torch.empty_like(x)
        L.check(l.dib_stem_pool_backward(go32.data_ptr(), arg32.data_ptr(), gx32.data_ptr(), N, H, W, C, L.stream_of(x)))
        gx = torch.full_like(x, 7.0)
        L.check(l.dib_stem_pool_backward_bf16(go.data_ptr(), arg32.data_ptr(), gx.data_ptr(), N, H, W, C, L.stream_of(x)))
        assert torch.equal(gx, gx32), (N, C, H, W)
    torch.cuda.synchronize()


# ---- fused nodes on bf16 against the plain-torch bf16 graph ---------------------------------------------------------------------

def _randomize_bn(m):
    from detectinblur_amd.models import backbone as B
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, B.FrozenBatchNorm2d):
                mod.weight.uniform_(0.5, 1.5); mod.bias.uniform_(-.2, .2); mod.running_mean.uniform_(-.2, .2); mod.running_var.uniform_(0.5, 1.5)


def _within_twice_the_plain_graphs_own_error(fused, plain, exact, what):
    """where MIOpen / a reduction may sum in another order: the bound is 2 x the plain bf16 graph's own distance from the same
    graph in float64 on the upcast inputs (same arithmetic, other summation order), computed here -- no constant"""
    own = float((plain.double() - exact.double().to(plain.device)).norm())
    err = float((fused.double() - plain.double()).norm())
    print("%s: |fused - plain| = %.3e, |plain - float64| = %.3e" % (what, err, own))
    assert err <= 2 * own, (what, err, own)


def test_bias_act_and_topdown_nodes_on_bf16_equal_the_plain_graph():
    from detectinblur_amd.models import backbone as B
    for k, shape in enumerate(((2, 64, 37, 53), (1, 256, 50, 84))):
        for res in (False, True):
            t, r, bias, g = _rand(shape, k, False), _rand(shape, 5 + k, False), _bias(shape[1], k), _rand(shape, 9 + k, False)
            t[0, :, 1, 2] = 0.0
            got = {}
            before = dict(B.LP_CALLS)
            try:
                for flag in (True, False):
                    B.FUSE_EPILOGUE = flag
                    a, rr, b0 = t.clone().requires_grad_(True), (r.clone().requires_grad_(True) if res else None), bias.clone().requires_grad_(True)
                    y = B.bias_act(a * 1.0, b0, rr, relu=True)
                    assert y.dtype == BF
                    y.backward(g)
                    got[flag] = (y.detach().clone(), a.grad.clone(), rr.grad.clone() if res else None, b0.grad.clone())
            finally:
                B.FUSE_EPILOGUE = True
            assert B.LP_CALLS["bias_act"] == before["bias_act"] + 1           # the bf16 kernel ran, once
            want = torch.relu(t.float() + bias.reshape(1, -1, 1, 1) + (r.float() if res else 0)).to(BF)
            assert torch.equal(got[False][0], want) and torch.equal(got[True][0], want)
            ref = torch.ops.aten.threshold_backward(g, want, 0)
            for flag in (True, False):
                assert torch.equal(got[flag][1], ref) and (not res or torch.equal(got[flag][2], ref))
                assert got[flag][3].dtype == torch.float32
            _within_twice_the_plain_graphs_own_error(got[True][3], got[False][3], ref.double().sum((0, 2, 3)), "bias gradient %s" % (shape,))
    for (N, C, H, W, Ht, Wt) in ((8, 256, 50, 84, 25, 42), (2, 256, 51, 101, 26, 51), (3, 8, 33, 20, 11, 7)):
        lat, top, bias, g = _rand((N, C, H, W), 1, False), _rand((N, C, Ht, Wt), 2, False), _bias(C, 3), _rand((N, C, H, W), 4, False)
        res = {}
        try:
            for flag in (True, False):
                B.FUSE_TOPDOWN = flag
                l0, t0, b0 = lat.clone().requires_grad_(True), top.clone().requires_grad_(True), bias.clone().requires_grad_(True)
                y = B.topdown_merge(l0 * 1.0, b0, t0)
                assert y.dtype == BF
                y.backward(g)
                res[flag] = (y.detach().clone(), l0.grad.clone(), t0.grad.clone(), b0.grad.clone())
        finally:
            B.FUSE_TOPDOWN = True
        for k in range(3):                                          # where the fp32 test asserts equality
            assert torch.equal(res[True][k], res[False][k]), (N, C, H, W, k)
        _within_twice_the_plain_graphs_own_error(res[True][3], res[False][3], g.double().sum((0, 2, 3)), "top-down bias gradient")


def test_entry_nodes_and_stem_on_bf16_against_the_plain_bf16_graph():
    """ResNet layer3 (a downsample block + five identity blocks) on a bf16 input with BLOCK_ENTRY on and off, and the whole body with the
    fused stem on and off: forward equal where the same kernels run, gradients within twice the plain bf16 graph's own distance
    from float64."""
    import copy
    from detectinblur_amd.models import backbone as B
    torch.manual_seed(2)
    body = B.ResNet50Body().cuda().to(memory_format=CL)
    _randomize_bn(body)
    exact = copy.deepcopy(body).cpu().double()
    x0 = _rand((2, 512, 20, 28), 3, False)

    def run(net, x, flag):
        B.BLOCK_ENTRY = flag
        x = x.clone().requires_grad_(True)
        for p in net.parameters():
            p.grad = None
        y = net.layer3(x)
        y.float().square().mean().backward() if y.dtype != torch.float64 else y.square().mean().backward()
        return [y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in net.layer3.parameters()]

    before = dict(B.LP_CALLS)
    try:
        run(body, x0, True); run(body, x0, False)
        fused, plain = run(body, x0, True), run(body, x0, False)
        truth = run(exact, x0.cpu().double().contiguous(memory_format=CL), False)
    finally:
        B.BLOCK_ENTRY = True
    assert B.LP_CALLS["block_entry"] == before["block_entry"] + 10 and B.LP_CALLS["down_entry"] == before["down_entry"] + 2
    assert fused[0].dtype == BF and fused[1].dtype == BF and all(g.dtype == torch.float32 for g in fused[2:])
    names = ["output", "input gradient"] + [n for n, _ in body.layer3.named_parameters()]
    for n, a, b, t in zip(names, fused, plain, truth):
        _within_twice_the_plain_graphs_own_error(a, b, t, "layer3 " + n)
    # the stem: pooled bf16 tensor bit for bit (same fp32 convolution in front of both), the body's outputs and conv1's gradient
    img = torch.randn(2, 3, 96, 128, device="cuda").contiguous(memory_format=CL)
    res = {}
    try:
        for flag in (True, False):
            B.FUSE_STEM_POOL = flag
            with torch.no_grad():
                res[flag, "stem"] = B.stem(img, body.conv1, body.bn1, BF)
            body.zero_grad()
            feats = body(img, BF)
            sum(f.float().square().mean() for f in feats).backward()
            res[flag] = [f.detach().clone() for f in feats] + [body.conv1.weight.grad.clone()]
    finally:
        B.FUSE_STEM_POOL = True
    assert res[True, "stem"].dtype == BF and torch.equal(res[True, "stem"], res[False, "stem"])
    exact.zero_grad()
    feats = exact(img.cpu().double())
    sum(f.square().mean() for f in feats).backward()
    truth = [f.detach() for f in feats] + [exact.conv1.weight.grad]
    for n, a, b, t in zip(["c2", "c3", "c4", "c5", "conv1.weight gradient"], res[True], res[False], truth):
        _within_twice_the_plain_graphs_own_error(a, b, t, "body " + n)


# ---- accuracy of the mode --------------------------------------------------------------------------------------------------------

_SWITCHES = ("FOLD_FROZEN_BN", "FUSE_EPILOGUE", "RELU_MASK", "LINEAR_1X1", "STRIDED_1X1_GEMM", "NCHW_SMALL_3X3", "BLOCK_ENTRY", "FOLD_ALL",
             "FUSE_TEST_TIME_BN", "PLANAR_FUSED", "FUSE_STEM_POOL", "FUSE_TOPDOWN")


@contextlib.contextmanager
def _stock():
    """the module-by-module trunk (every switch of backbone.py off, the RPN head's too)"""
    from detectinblur_amd.models import backbone as B
    from detectinblur_amd.models import rpn as R
    old = {k: getattr(B, k) for k in _SWITCHES}
    old_head = R.FUSE_HEAD
    try:
        for k in _SWITCHES:
            setattr(B, k, False)
        R.FUSE_HEAD = False
        yield
    finally:
        for k, v in old.items():
            setattr(B, k, v)
        R.FUSE_HEAD = old_head


@pytest.mark.parametrize("size", [(128, 160), (800, 1344)], ids=["toy", "full"])
def test_trunk_accuracy_against_stock_autocast(size):
    """fp32 trunk of this model = truth; reference = stock PyTorch (module-by-module trunk under torch.autocast bf16), measured in this
    run.  Per FPN level |y - y32|_inf / |y32|_inf, per trainable convolution weight |g - g32|_2 / |g32|_2 for the loss
    sum_levels (y * r).sum(): amp <= 4 x reference for each (autocast keeps the skip path and the batch-norm output in fp32
    between convolutions, this mode stores them in bf16: one more rounding of relative size 2^-9 per bottleneck along 16)."""
    from detectinblur_amd.models import backbone as B
    torch.manual_seed(11)
    net = B.resnet_fpn_backbone("resnet50", False, trainable_layers=5).cuda().to(memory_format=CL)
    _randomize_bn(net)
    x = torch.randn(1, 3, *size, device="cuda").contiguous(memory_format=CL)
    convs = [(n, p) for n, p in net.named_parameters() if p.dim() == 4]
    assert len(convs) == 53 + 8

    def run(mode, r):
        for p in net.parameters():
            p.grad = None
        net.compute_dtype = BF if mode == "amp" else torch.float32
        try:
            if mode == "stock":
                with _stock(), torch.autocast("cuda", BF):
                    out = net(x)
            else:
                out = net(x)
        finally:
            net.compute_dtype = torch.float32
        out = {k: v.float() for k, v in out.items()}
        if r is None:
            g = torch.Generator(device="cuda").manual_seed(5)
            r = {k: torch.randn(v.shape, device="cuda", generator=g) for k, v in out.items()}
        sum((out[k] * r[k]).sum() for k in out).backward()
        return {k: v.detach() for k, v in out.items()}, {n: p.grad.clone() for n, p in convs}, r

    y32, g32, r = run("fp32", None)
    ya, ga, _ = run("amp", r)
    ys, gs, _ = run("stock", r)
    rows, bad = [], []
    for k in y32:
        a = float((ya[k] - y32[k]).abs().max() / y32[k].abs().max())
        s = float((ys[k] - y32[k]).abs().max() / y32[k].abs().max())
        rows.append(("level " + k, a, s))
    for n, _ in convs:
        a = float((ga[n] - g32[n]).norm() / g32[n].norm())
        s = float((gs[n] - g32[n]).norm() / g32[n].norm())
        rows.append((n, a, s))
    print("trunk accuracy at 1 x 3 x %d x %d: tensor, amp, stock autocast, ratio" % size)
    for name, a, s in rows:
        print("  %-40s %.4e %.4e %.2f" % (name, a, s, a / s if s > 0 else float("inf")))
        assert a == a and s == s and s > 0, name
        if not a <= 4 * s:
            bad.append((name, a, s))
    assert not bad, bad


def _toy_detector(compute_dtype=torch.float32):
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    torch.manual_seed(0)
    return fasterrcnn_resnet50_fpn(pretrained=False, pretrained_backbone=False, num_classes=91, min_size=320, max_size=480,
                                   compute_dtype=compute_dtype).cuda()


def test_losses_against_stock_autocast():
    """One model in train mode, three seeded batches of two images, forward only: the four loss terms each, 12 numbers per mode;
    sum |amp - fp32| <= 4 x sum |stock - fp32|, the stock reference (module-by-module trunk and RPN head under torch.autocast,
    the scope of the mode) run here."""
    m = _toy_detector().train()
    means, stds = np.tile([0.485, 0.456, 0.406], (2, 1)), np.tile([0.229, 0.224, 0.225], (2, 1))
    body_fwd, head_fwd = m.backbone.forward, m.rpn.head.forward

    def cast_backbone(x):
        with torch.autocast("cuda", BF):
            out = body_fwd(x)
        return type(out)((k, v.float()) for k, v in out.items())

    def cast_head(feats):
        with torch.autocast("cuda", BF):
            logits, deltas = head_fwd(feats)
        return [t.float() for t in logits], [t.float() for t in deltas]

    def losses(mode):
        out = []
        for b in range(3):
            g = torch.Generator().manual_seed(40 + b)
            imgs = [torch.rand(3, 320, 480, generator=g).cuda(), torch.rand(3, 300, 440, generator=g).cuda()]
            tg = [{"boxes": torch.tensor([[30., 40., 200., 260.], [100., 20., 300., 180.]]).cuda(), "labels": torch.tensor([3, 17]).cuda()},
                  {"boxes": torch.tensor([[10., 50., 150., 290.]]).cuda(), "labels": torch.tensor([44]).cuda()}]
            torch.manual_seed(100 + b)                              # the samplers' draws
            m.backbone.compute_dtype = BF if mode == "amp" else torch.float32
            try:
                with torch.no_grad():
                    if mode == "stock":
                        m.backbone.forward, m.rpn.head.forward = cast_backbone, cast_head
                        with _stock():
                            d = m(imgs, tg, newMeans=means, newSTDs=stds)
                    else:
                        d = m(imgs, tg, newMeans=means, newSTDs=stds)
            finally:
                m.backbone.compute_dtype = torch.float32
                m.backbone.__dict__.pop("forward", None); m.rpn.head.__dict__.pop("forward", None)
            out += [float(d[k]) for k in ("loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg")]
        return np.array(out)

    l32, la, ls = losses("fp32"), losses("amp"), losses("stock")
    assert len(l32) == 12 and np.isfinite(la).all() and np.isfinite(ls).all()
    da, ds = float(np.abs(la - l32).sum()), float(np.abs(ls - l32).sum())
    print("losses fp32 %s\n       amp  %s\n       stock %s\nsum|amp - fp32| = %.4e, sum|stock - fp32| = %.4e" % (l32, la, ls, da, ds))
    assert da <= 4 * ds, (da, ds)


# ---- graphed inference -----------------------------------------------------------------------------------------------------------

def _det_equal(a, b):
    return all(x[k].shape == y[k].shape and torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in ("boxes", "labels", "scores"))


def test_graphed_inference_with_amp_equals_eager_and_follows_a_weight_update():
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    torch.manual_seed(0)
    m = fasterrcnn_resnet50_fpn(pretrained=False, pretrained_backbone=False, num_classes=91, compute_dtype=BF).cuda().eval()
    m.roi_heads.score_thresh = 0.0
    torch.manual_seed(1)
    images = [torch.rand(3, 800, 1333, device="cuda"), torch.rand(3, 600, 800, device="cuda")]
    means, stds = np.tile([0.485, 0.456, 0.406], (1, 1)), np.tile([0.229, 0.224, 0.225], (1, 1))
    order = [0, 1, 0, 1]

    def passes(graph):
        m.graph_inference = graph
        with torch.no_grad():
            return [[{k: v.clone() for k, v in d.items()} for d in m([images[i]], newMeans=means, newSTDs=stds)] for i in order]

    eager, eager2 = passes(False), passes(False)
    assert all(_det_equal(a, b) for a, b in zip(eager, eager2))                     # the eager bf16 path itself is reproducible
    graphed, again = passes(True), passes(True)
    cache = m._trunk_graphs
    assert len(cache.graphs) == 2 and all(g is not None for g in cache.graphs.values())
    assert len(eager[0][0]["boxes"]) > 0
    for e, g, a in zip(eager, graphed, again):
        assert _det_equal(e, g) and _det_equal(e, a)
    lp = [c for c in m.backbone.body.modules() if "_dib_fold_lp" in c.__dict__]       # every body convolution but the fp32 stem's
    assert len(lp) == 52 and all(c.__dict__["_dib_fold_lp"][1].dtype == BF for c in lp)
    graphs = dict(cache.graphs)
    opt = torch.optim.SGD(m.parameters(), lr=1.0)
    for p in m.parameters():
        p.grad = torch.randn_like(p) * 0.05 * p.detach().abs().mean().clamp(min=1e-3)
    opt.step()
    m.eval()
    e1, g1 = passes(False), passes(True)
    assert all(cache.graphs[k] is v for k, v in graphs.items())                     # same graphs, folds rewritten in place
    for e, g in zip(e1, g1):
        assert _det_equal(e, g)
    k = min(3, len(e1[0][0]["scores"]), len(eager[0][0]["scores"]))
    assert k > 0 and not torch.allclose(e1[0][0]["scores"][:k], eager[0][0]["scores"][:k], atol=1e-2)       # the step moved the detector


def test_bf16_inference_convolutions_through_conv1x1_are_bit_reproducible():
    """Every convolution shape of the b = 1 trunk and RPN head at 800 x 1344, bf16, without autograd, through backbone.conv1x1 (GEMM
    for 1x1, im2col + GEMM for 3x3 up to 16,800 output pixels, MIOpen's channels-last kernels for the larger 3x3): five runs on the
    same input are equal -- what a replayed graph needs.  The im2col + GEMM form is held to the convolution it replaces: its distance
    from the float64 convolution of the upcast operands is at most twice that of MIOpen's bf16 kernel (same arithmetic, other
    summation order).  Checked on the strided shapes and the two smallest, where the float64 convolution is cheap."""
    import types
    from detectinblur_amd.models import backbone as B
    shapes = [(64, 256, 200, 1, 1), (64, 64, 200, 1, 1), (64, 64, 200, 3, 1), (256, 64, 200, 1, 1), (256, 512, 200, 1, 2), (256, 128, 200, 1, 1),
              (128, 128, 200, 3, 2), (128, 512, 100, 1, 1), (512, 128, 100, 1, 1), (128, 128, 100, 3, 1), (512, 1024, 100, 1, 2), (512, 256, 100, 1, 1),
              (256, 256, 100, 3, 2), (256, 1024, 50, 1, 1), (1024, 256, 50, 1, 1), (256, 256, 50, 3, 1), (1024, 2048, 50, 1, 2), (1024, 512, 50, 1, 1),
              (512, 512, 50, 3, 2), (512, 2048, 25, 1, 1), (2048, 512, 25, 1, 1), (512, 512, 25, 3, 1), (2048, 256, 25, 1, 1), (256, 256, 25, 3, 1),
              (256, 256, 100, 3, 1), (256, 256, 200, 1, 1), (256, 256, 200, 3, 1), (256, 256, 13, 3, 1)]
    widths = {200: 336, 100: 168, 50: 84, 25: 42, 13: 21}
    g = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():
        for ci, co, h, k, s in shapes:
            conv = types.SimpleNamespace(kernel_size=(k, k), stride=(s, s), padding=(k // 2, k // 2), dilation=(1, 1), groups=1, in_channels=ci, out_channels=co)
            x = torch.randn((1, ci, h, widths[h]), device="cuda", generator=g).to(BF).contiguous(memory_format=CL)
            w = (torch.randn((co, ci, k, k), device="cuda", generator=g) * (2.0 / (ci * k * k)) ** 0.5).to(BF).contiguous(memory_format=CL)
            ys = [B.conv1x1(x, w, None, conv).clone() for _ in range(5)]
            assert ys[0].dtype == BF and ys[0].is_contiguous(memory_format=CL)
            assert all(torch.equal(ys[0], y) for y in ys[1:]), (ci, co, h, k, s)
            ho = (h + 2 * (k // 2) - k) // s + 1
            assert B._as_unfold_gemm(x, conv) == (k == 3 and ho * ((widths[h] + 2 * (k // 2) - k) // s + 1) <= 16800)
            if k == 3 and (s == 2 or h <= 25):
                exact = F.conv2d(x.cpu().double(), w.cpu().double(), None, s, 1)
                plain = F.conv2d(x, w, None, s, 1)
                _within_twice_the_plain_graphs_own_error(ys[0], plain, exact, "im2col + GEMM %d -> %d at %d" % (ci, co, h))


# ---- drivers ---------------------------------------------------------------------------------------------------------------------

def _train_child(argv, ckpt):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from detectinblur_amd import train
    from detectinblur_amd.models import backbone as B
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train.main(train.build_parser().parse_args(list(argv)))
    text = buf.getvalue()
    state = torch.load(ckpt, map_location="cpu", weights_only=False)
    return {"losses": [float(x) for x in re.findall(r"  loss: ([0-9.eE+-]+|nan|inf)", text)], "lp_calls": dict(B.LP_CALLS),
            "dtypes": sorted({str(v.dtype) for v in state["model"].values() if v.is_floating_point()}),
            "momentum": sorted({str(s["momentum_buffer"].dtype) for s in state["optimizer"]["state"].values() if s.get("momentum_buffer") is not None}),
            "amp": bool(state["args"].amp), "tail": text[-400:]}


def train_child(out_path, argv, ckpt):
    from tests import _gpu_children
    _gpu_children._guarded(_train_child, out_path, (argv, ckpt))


def test_train_main_with_amp_in_a_fresh_child(tmp_path):
    from tests.test_ddp_gpu import _run_child
    steps = 3
    argv = ["--synthetic", "--synthetic_images", str(2 * (steps + 1)), "--blur_train", "--gpu_blur", "--expand_target_boxes", "-b", "2", "--amp",
            "--epochs", "1", "--early_stop", str(steps), "--lr", "0.002", "--print_freq", "1", "--output_dir", str(tmp_path / "w"),
            "--tensorboard_path", ""]
    r = _run_child(train_child, tmp_path, argv, str(tmp_path / "w" / "model_0.pth"))
    assert r["amp"] and len(r["losses"]) >= steps - 1 and all(np.isfinite(r["losses"])), r
    assert r["dtypes"] == ["torch.float32"] and r["momentum"] == ["torch.float32"], r
    n = r["lp_calls"]["down_entry"] // 4                        # training forward passes (the entry nodes only exist under autograd)
    assert n >= steps and r["lp_calls"]["stem_pool"] >= n
    # per training pass every bias_act of the trunk took the bf16 kernel: 16 bottlenecks x 3 + 4 downsample shifts, 4 FPN output
    # biases + the top lateral's, 5 RPN head levels; the 3 other laterals' biases ride on the top-down merge
    assert r["lp_calls"]["block_entry"] == 12 * n and r["lp_calls"]["down_entry"] == 4 * n and r["lp_calls"]["topdown_merge"] >= 3 * n, r
    assert r["lp_calls"]["bias_act"] >= (16 * 3 + 4 + 5 + 5) * n, r


def test_evaluate_main_sweep_with_amp(tmp_path, capsys):
    """15 cells, 12 statistic lines each.  Run-to-run identity of the statistics is not asserted under --amp: the shipped find-db
    holds fp32 records only, so MIOpen picks its bf16 solvers by its own search on the running stack."""
    from detectinblur_amd import evaluate as E
    res = E.main(E.build_parser().parse_args(["--synthetic", "--synthetic_images", "3", "--amp", "--blur_eval", "--gpu_blur", "--early_stop", "3",
                                              "--tensorboard_path", ""]))
    text = capsys.readouterr().out
    assert len(res) == 15 and all(len(v.coco_eval["bbox"].stats) == 12 for v in res.values())
    assert len([l for l in text.splitlines() if "Average Precision" in l or "Average Recall" in l]) == 12 * 15
    assert "amp=True" in text
