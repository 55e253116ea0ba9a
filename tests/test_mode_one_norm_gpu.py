"""`--mode_one_norm` on the MI355X: the HIP path of models/batchnorm.BatchNorm2d (csrc/dib_bnstats.hip) against float64 on the
53 trunk shapes at batch 1, 800 x 1344 (and N = 2), against the fixture's reference outputs, and bitwise against itself; the
same bounds on small shapes that reach every branch of the launch geometry, and a NaN that stays in its channel; the
converted detector (every layer on the HIP path, close to the torch path, graphed == eager, conversion after a frozen
evaluation == a fresh conversion); and evaluate.main --mode_one_norm reproducible across two fresh processes."""
import copy

import numpy as np
import pytest
import torch

from detectinblur_amd import utils
from detectinblur_amd.models import backbone
from detectinblur_amd.models.batchnorm import BatchNorm2d

pytestmark = pytest.mark.gpu

N_TRACKED = 16


def _trunk_shapes():
    """(C, H, W, residual, relu) of the 53 batch-norm layers of ResNet-50 at 800 x 1344 (stem, then stage by stage)."""
    out = [(64, 400, 672, False, True)]
    hw = (200, 336)
    for planes, blocks, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)):
        H, W = hw
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        for b in range(blocks):
            hin = (H, W) if b == 0 else (Ho, Wo)
            out.append((planes, hin[0], hin[1], False, True))          # bn1 behind the 1x1
            out.append((planes, Ho, Wo, False, True))                  # bn2 behind the (strided) 3x3
            out.append((planes * 4, Ho, Wo, True, True))               # bn3: + identity, ReLU
            if b == 0:
                out.append((planes * 4, Ho, Wo, False, False))         # downsample
        hw = (Ho, Wo)
    assert len(out) == 53
    return out


SHAPES = sorted(set(_trunk_shapes()))


def _layer(C, dev, seed):
    g = torch.Generator().manual_seed(seed)
    bn = BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.rand(C, generator=g) - 0.5)
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) * 2 + 0.2)
    bn.num_batches_tracked = bn.num_batches_tracked + N_TRACKED
    bn.mode_one = True
    return bn.to(dev).eval()


def _activation(N, C, H, W, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    mean = torch.randn((1, C, 1, 1), generator=g, device=dev) * 3
    std = torch.rand((1, C, 1, 1), generator=g, device=dev) * 2 + 0.1
    x = torch.randn((N, C, H, W), generator=g, device=dev) * std + mean
    return x.contiguous(memory_format=torch.channels_last)


def _f64(bn, x, res, relu):
    x64 = x.double()
    C = x.shape[1]
    xs = x64.permute(1, 0, 2, 3).reshape(C, -1)
    mb, vb = xs.mean(1), xs.var(1, unbiased=False)
    n = float(bn.num_batches_tracked)
    f, g = n / (n + 1), 1 / (n + 1)
    mean = f * bn.running_mean.double() + g * mb
    var = f * bn.running_var.double() + g * vb
    scale = bn.weight.double() / torch.sqrt(var + bn.eps)
    y = (x64 - mean.view(1, -1, 1, 1)) * scale.view(1, -1, 1, 1) + bn.bias.double().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double()
    if relu:
        y = y.clamp_min(0)
    return mean, var, y


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "C%d_%dx%d%s%s" % (s[0], s[1], s[2], "_res" if s[3] else "", "_relu" if s[4] else ""))
def test_kernel_against_float64_on_the_trunk_shapes(shape, N):
    C, H, W, has_res, relu = shape
    if N == 2 and C * H * W > 256 * 200 * 336:
        pytest.skip("N = 2 is covered from layer1 down")
    dev = torch.device("cuda")
    bn = _layer(C, dev, C + H)
    x = _activation(N, C, H, W, dev, 7 * C + W)
    for res_on, relu_on in {(has_res, relu), (False, False), (True, True)}:
        res = _activation(N, C, H, W, dev, 11 * C + H) if res_on else None
        stats = torch.empty((2, C), dtype=torch.float32, device=dev)
        y = bn._mode_one_hip_(x.clone(memory_format=torch.channels_last), res, relu_on, stats)
        y2 = bn._mode_one_hip_(x.clone(memory_format=torch.channels_last), res, relu_on)
        torch.cuda.synchronize()
        assert torch.equal(y, y2), "two calls on the same input differ"
        mean64, var64, y64 = _f64(bn, x, res, relu_on)
        sd = var64.sqrt()
        # the mean: 1e-5 sigma, or two fp32 ulps of |mean| where that is larger (the mixed mean is ONE fp32 number)
        assert bool(((stats[0].double() - mean64).abs() <= 1e-5 * sd + 2.4e-7 * mean64.abs()).all())
        assert bool(((stats[1].double() - var64).abs() <= 1e-5 * var64).all())
        err = (y.detach().double() - y64).abs() / (1 + y64.abs())
        assert float(err.max()) <= 1e-4, float(err.max())


def test_kernel_against_the_fixture():
    from tests.test_mode_one_norm import CASES, fixture_case, load_fixture
    fx = load_fixture()
    dev = torch.device("cuda")
    for name, *_ in CASES:
        d = fixture_case(fx, name)
        C = d["running_mean"].shape[0]
        bn = BatchNorm2d(C)
        with torch.no_grad():
            for k in ("weight", "bias", "running_mean", "running_var"):
                getattr(bn, k).copy_(torch.from_numpy(d[k]))
        bn.num_batches_tracked = bn.num_batches_tracked + int(fx["num_batches_tracked"])
        bn.mode_one = True
        bn = bn.to(dev).eval()
        x = torch.from_numpy(d["x"]).to(dev).contiguous(memory_format=torch.channels_last)
        stats = torch.empty((2, C), dtype=torch.float32, device=dev)
        with torch.no_grad():
            y = bn._mode_one_hip_(x.clone(memory_format=torch.channels_last), None, False, stats)
            y_mod = bn(x)
        assert bn.last_path == "hip"
        assert torch.equal(y, y_mod)
        y = y.cpu().double().numpy()
        y64, y_ref = fx[name + "/y64"], fx[name + "/y_ref"].astype(np.float64)
        assert np.all(np.abs(y - y64) <= 1e-4 * (1 + np.abs(y64))), name
        assert np.all(np.abs(y - y_ref) <= 1e-4 * (1 + np.abs(y_ref))), name
        var64 = fx[name + "/var64"]
        assert np.all(np.abs(stats[1].cpu().double().numpy() - var64) <= 1e-5 * var64), name      # incl. |mean| ~ 1e3 sigma


def test_num_batches_tracked_on_the_host_or_the_device():
    dev = torch.device("cuda")
    bn = _layer(64, dev, 3)
    x = _activation(1, 64, 30, 40, dev, 4)
    a = bn._mode_one_hip_(x.clone(memory_format=torch.channels_last))
    bn.num_batches_tracked = bn.num_batches_tracked.cpu()
    b = bn._mode_one_hip_(x.clone(memory_format=torch.channels_last))
    assert torch.equal(a, b)


# ---- launch geometry between the fixture's tiny cases and the trunk shapes, and a NaN ---------------------------------------------

# (C, npix) chosen from bn_geometry (csrc/dib_bnstats.hip) so that every branch of it is reached; R = pixel rows per workgroup,
# QB = channel quads per workgroup, S = pixel slices
GEOMETRY = [(4, 1), (4, 1023), (4, 4096), (4, 8195),      # R = 1024: one pixel; idle rows; S = 1 exactly; S = 2 with uneven slices
            (12, 2731),                                    # QB = 3, R = 341: lane 1023 idle; S = 2
            (260, 197),                                    # two channel chunks, the second with one live quad; S = 3
            (64, 16401), (64, 16643), (64, 65791)]         # S = 64, 65 (the finalize batch boundary) and the cap of 256


def _relu_keeping_nan(y):
    """the ReLU of the epilogue references, oracle/dib_oracle.py relu32 itself (numpy, on the host)"""
    import dib_oracle as O
    return torch.from_numpy(O.relu32(y.cpu().numpy())).to(y.device)


def _geometry_input(C, npix, dev, seed):
    """[1, C, npix, 1] channels-last: _activation's channels, with channel 0 constant (batch variance exactly 0), channel 1 a
    narrow channel with one outlier and, for npix <= 8195, channel 2 at |mean| ~ 1e3 sigma.  The kernel reports the MIXED
    statistics only (16/17 running + 1/17 batch), so the zero batch variance is checked through that mix: an error e of the
    batch variance shows as e / 17 against a bound of 1e-5 of the mixed variance."""
    x = _activation(1, C, npix, 1, dev, seed)
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    x[:, 0] = 3.25
    x[:, 1] = torch.randn((1, npix, 1), generator=g, device=dev) * 0.01
    x[0, 1, npix // 3, 0] = 1000.0
    if npix <= 8195:
        x[:, 2] = torch.randn((1, npix, 1), generator=g, device=dev) + 1000.0
    return x


def _check_against_float64(bn, x, res, relu_on, channels=None, what=None):
    stats = torch.empty((2, x.shape[1]), dtype=torch.float32, device=x.device)
    y = bn._mode_one_hip_(x.clone(memory_format=torch.channels_last), res, relu_on, stats)
    y2 = bn._mode_one_hip_(x.clone(memory_format=torch.channels_last), res, relu_on)
    torch.cuda.synchronize()
    with torch.no_grad():
        mean64, var64, y64 = _f64(bn, x, res, False)
    if relu_on:
        y64 = _relu_keeping_nan(y64)
    c = slice(None) if channels is None else channels
    assert torch.equal(y[:, c], y2[:, c]), "two calls on the same input differ"
    sd = var64.sqrt()
    em = ((stats[0].double() - mean64).abs() / (1e-5 * sd + 2.4e-7 * mean64.abs()))[c]
    ev = ((stats[1].double() - var64).abs() / (1e-5 * var64))[c]
    ey = ((y.detach().double() - y64).abs() / (1 + y64.abs()))[:, c]
    print("%s: mean error / bound %.3f (channel %d), variance error / bound %.3f (channel %d), output error %.2e"
          % (what, float(em.max()), int(em.argmax()), float(ev.max()), int(ev.argmax()), float(ey.max())))
    assert float(em.max()) <= 1, (what, "mean", em.tolist()[:4])
    assert float(ev.max()) <= 1, (what, "variance", ev.tolist()[:4])
    assert float(ey.max()) <= 1e-4, (what, float(ey.max()))
    return stats, y


@pytest.mark.parametrize("C,npix", GEOMETRY, ids=lambda v: str(v))
def test_kernel_against_float64_across_the_launch_geometry(C, npix):
    """The file's bounds (mean 1e-5 sigma + 2.4e-7 |mean|, variance 1e-5 relative, output 1e-4 (1 + |y|)) on every branch of the
    partial-statistics geometry, with and without residual and ReLU, including a constant, a one-outlier and a large-mean channel."""
    dev = torch.device("cuda")
    bn = _layer(C, dev, C + npix % 97)
    x = _geometry_input(C, npix, dev, 7 * C + npix % 89)
    r = _activation(1, C, npix, 1, dev, 11 * C + npix % 83)
    for res_on in (False, True):
        for relu_on in (False, True):
            _check_against_float64(bn, x, r if res_on else None, relu_on, what="C %d, %d pixels%s%s" % (C, npix, ", residual" if res_on else "", ", relu" if relu_on else ""))


def test_a_nan_poisons_its_channel_only_and_passes_the_relu():
    """C = 8, 63 pixels, a single NaN in channel 5: channel 5 of the output is NaN everywhere, with the ReLU on and off (torch's relu
    keeps a NaN), its statistics are NaN; the other channels -- the three that share channel 5's float4 included -- stay within
    the bounds."""
    dev = torch.device("cuda")
    C, npix = 8, 63
    bn = _layer(C, dev, 5)
    x = _activation(1, C, 7, 9, dev, 6)
    x[0, 5, 3, 4] = float("nan")
    r = _activation(1, C, 7, 9, dev, 8)
    others = [0, 1, 2, 3, 4, 6, 7]
    for res_on in (False, True):
        for relu_on in (False, True):
            stats, y = _check_against_float64(bn, x, r if res_on else None, relu_on, channels=others, what="NaN case, relu %d, residual %d" % (relu_on, res_on))
            assert bool(torch.isnan(stats[:, 5]).all()), stats[:, 5]
            assert bool(torch.isnan(y[:, 5]).all()), (relu_on, int(torch.isnan(y[:, 5]).sum()), npix)
            assert not bool(torch.isnan(y[:, others]).any())


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

# the argument lists of include/dib.h, by name, so that a row of a refusal table names what it changes
_BN_HEAD = ("x", "residual", "n_pix", "C", "weight", "bias", "running_mean", "running_var", "num_batches_dev")
_BN_TAIL = ("eps", "relu", "workspace", "workspace_bytes", "stats", "stream")
BN_ARGUMENTS = {"dib_bn_mode_one_nhwc": _BN_HEAD + ("num_batches",) + _BN_TAIL,
                "dib_bn_acclimate_nhwc": _BN_HEAD + ("bump", "momentum") + _BN_TAIL}
NEEDS_SHAPE = "needs n_pix > 0 and C % 4 == 0"
NULL_POINTER = "null pointer"
ALIGNED_16 = "x, residual and workspace must be 16-byte aligned"


def refusal_case(dev, **own):
    """A valid call on C = 8, two pixels ([1, 8, 2, 1] channels-last, flat) as a dictionary of arguments, `own` being the entry
    point's own ones; the tensors behind it -- every buffer four elements longer than the call needs, so that a pointer moved
    by 4 bytes still points into it -- and the refusals both entry points share: (what, changed arguments, code, fragment)."""
    from detectinblur_amd import _lib
    g = torch.Generator().manual_seed(9)
    C, npix = 8, 2
    need = _lib.lib().dib_bn_mode_one_workspace_bytes(npix, C)
    t = {k: torch.randn(n + 4, generator=g).to(dev) for k, n in (("x", C * npix), ("residual", C * npix), ("weight", C), ("bias", C), ("running_mean", C))}
    t["running_var"] = (torch.rand(C + 4, generator=g) + 0.5).to(dev)
    t["workspace"] = torch.zeros(need // 4 + 4, dtype=torch.float32, device=dev)
    t["counter"] = torch.full((2,), N_TRACKED, dtype=torch.int64, device=dev)
    p = {k: v.data_ptr() for k, v in t.items()}
    base = dict(x=p["x"], residual=None, n_pix=npix, C=C, weight=p["weight"], bias=p["bias"], running_mean=p["running_mean"],
                running_var=p["running_var"], num_batches_dev=p["counter"], eps=1e-5, relu=0, workspace=p["workspace"], workspace_bytes=need,
                stats=None, stream=_lib.stream_of(t["x"]), **own)
    E = _lib.DIB_EINVAL
    rows = [("C = 6", dict(C=6), E, NEEDS_SHAPE + " (C = 6)"), ("no pixels", dict(n_pix=0), E, NEEDS_SHAPE + " (C = 8)")]
    rows += [(k + " null", {k: None}, E, NULL_POINTER) for k in ("x", "running_mean", "running_var", "workspace")]
    rows += [(k + " + 4 bytes", {k: p[k] + 4}, E, ALIGNED_16) for k in ("x", "residual", "workspace")]
    rows += [("workspace one byte short", dict(workspace_bytes=need - 1), E, "workspace of %d bytes, needs %d" % (need - 1, need))]
    return base, t, rows


def check_refusals(entry, base, tensors, rows):
    """Every row is refused with its code and a message that names `entry` and holds the row's fragment, and after a
    synchronise x, both running buffers and the counter hold the bits they held.  Then the unchanged call is accepted."""
    from detectinblur_amd import _lib
    l = _lib.lib()
    watched = [tensors[k] for k in ("x", "running_mean", "running_var", "counter")]
    before = [w.clone() for w in watched]
    for what, change, code, fragment in rows:
        assert set(change) <= set(base), what
        args = dict(base, **change)
        rc = getattr(l, entry)(*[args[k] for k in BN_ARGUMENTS[entry]])
        text = l.dib_last_error().decode()
        torch.cuda.synchronize()
        assert rc == code and text.startswith(entry + ": ") and fragment in text, (what, rc, text)
        for w, b in zip(watched, before):
            assert torch.equal(w.view(torch.uint8), b.view(torch.uint8)), what
    _lib.check(getattr(l, entry)(*[base[k] for k in BN_ARGUMENTS[entry]]))
    torch.cuda.synchronize()


def test_entry_point_refusals_name_their_fault_and_launch_nothing():
    from detectinblur_amd import _lib
    base, tensors, rows = refusal_case(torch.device("cuda"), num_batches=N_TRACKED)
    rows += [("no counter on the device and a negative one on the host", dict(num_batches_dev=None, num_batches=-1), _lib.DIB_EINVAL,
              "negative num_batches_tracked")]
    check_refusals("dib_bn_mode_one_nhwc", base, tensors, rows)


# ---- the converted detector ----------------------------------------------------------------------------------------------------------

def _detector():
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    torch.manual_seed(0)
    m = fasterrcnn_resnet50_fpn(num_classes=91, pretrained=False, pretrained_backbone=False)
    g = torch.Generator().manual_seed(1)
    for mod in m.modules():
        if isinstance(mod, backbone.FrozenBatchNorm2d):
            C = mod.weight.shape[0]
            mod.weight.copy_(torch.rand(C, generator=g) + 0.5)
            mod.bias.copy_(torch.rand(C, generator=g) - 0.5)
            mod.running_mean.copy_(torch.rand(C, generator=g) - 0.5)
            mod.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    return m.to("cuda").eval()


def _convert(m):
    m = utils.convert_to_custom_batch_norm(m, batch_norm_to_use=BatchNorm2d)
    m = utils.set_batch_norm_N(m, 16)
    m = utils.set_batch_norm_mode1(m, True)
    return m.eval()           # the new layers start in training mode, where the reference also bumps num_batches_tracked


def _image():
    g = torch.Generator().manual_seed(2)
    return torch.rand((3, 800, 1333), generator=g).cuda()


def _features(m, img):
    with torch.no_grad():
        batch, _ = m.transform([img])
        return m.backbone(batch.tensors)


def test_converted_trunk_runs_every_layer_on_the_hip_path_close_to_the_torch_path():
    m = _convert(_detector())
    img = _image()
    bns = [b for b in m.modules() if isinstance(b, BatchNorm2d)]
    assert len(bns) == 53
    for b in bns:
        b.last_path = None
    fast = _features(m, img)
    assert [b.last_path for b in bns] == ["hip"] * 53
    assert all(b.num_batches_tracked.is_cuda for b in bns)
    old = backbone.FUSE_TEST_TIME_BN
    backbone.FUSE_TEST_TIME_BN = False
    try:
        slow = _features(m, img)
    finally:
        backbone.FUSE_TEST_TIME_BN = old
    assert [b.last_path for b in bns] == ["torch"] * 53
    for k in fast:
        rel = float((fast[k] - slow[k]).abs().max()) / float(slow[k].abs().max())
        assert rel <= 1e-3, (k, rel)


def _detections(m, img, graphed):
    m.graph_inference = graphed
    with torch.no_grad():
        outs = [m([img])[0] for _ in range(3)]        # the graph cache captures on a later sighting
    torch.cuda.synchronize()
    return outs[-1]


def test_graphed_trunk_equals_eager_and_conversion_after_a_frozen_run_equals_a_fresh_one():
    img = _image()
    fresh = _convert(_detector())
    eager = _detections(fresh, img, False)
    graphed = _detections(fresh, img, True)
    assert "_trunk_graphs" in fresh.__dict__
    for k in ("boxes", "scores", "labels"):
        assert torch.equal(eager[k], graphed[k]), k
    late = _detector()
    frozen = _detections(late, img, True)                 # captured with frozen batch-norm
    late = _convert(late)
    again = _detections(late, img, True)
    for k in ("boxes", "scores", "labels"):
        assert torch.equal(again[k], graphed[k]), k
    assert not (frozen["boxes"].shape == again["boxes"].shape and torch.equal(frozen["boxes"], again["boxes"]))


# ---- driver ----------------------------------------------------------------------------------------------------------------------------

def evaluate_main_digest_child(out_path, argv):
    from tests import _gpu_children
    _gpu_children._guarded(_gpu_children._evaluate_main_digest, out_path, (argv,))


def test_two_runs_of_evaluate_main_mode_one_print_identical_coco_stats(tmp_path):
    from tests.test_ddp_gpu import _run_child
    argv = ["--synthetic", "--synthetic_images", "3", "--mode_one_norm", "--blur_eval", "--gpu_blur", "--early_stop", "3"]
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    a = _run_child(evaluate_main_digest_child, tmp_path / "a", argv)
    b = _run_child(evaluate_main_digest_child, tmp_path / "b", argv)
    assert len(a["stat_lines"]) == 12 * 15
    assert a["stat_lines"] == b["stat_lines"]
    for cell in a["cells"]:
        assert a["cells"][cell] == b["cells"][cell], cell
