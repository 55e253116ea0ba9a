"""`--acclimate_norm` on the MI355X: dib_bn_acclimate_nhwc (csrc/dib_bnstats.hip) against float64 on shapes that reach every
branch of the launch geometry -- batch statistics, the updated running pair written in place, the counter bumped in place, the
output; both averaging rules, with and without the bump -- and bitwise against itself; an eight-step sequence that carries the
state; one pixel; a NaN that stays in its channel; the converted toy-size trunk (every layer on the HIP path, close to the
torch path); graphed == eager and pipelined == plain, bit for bit in detections and final buffers (a process of its own, MIOpen
in deterministic mode); evaluate.main --acclimate_norm reproducible across two fresh processes.

Bounds (the statistics kernels reorder sums, so they are held to float64, not to ATen's fp32; tests/test_mode_one_norm_gpu.py):
batch mean 1e-5 sigma_b + 2.4e-7 |mean_b|; variances 1e-5 relative; updated running mean 1e-5 sigma_b + 2.4e-7 max(|rm|, |mean_b|)
(the two products may cancel); updated running variance 1e-5 max(rv, var_u); outputs 1e-4 (1 + |y|)."""
import copy

import pytest
import torch

from detectinblur_amd import _lib, utils
from detectinblur_amd.models import backbone
from detectinblur_amd.models.batchnorm import BatchNorm2d
from tests.test_mode_one_norm_gpu import ALIGNED_16, _activation, _geometry_input, _relu_keeping_nan, check_refusals, refusal_case

pytestmark = pytest.mark.gpu

PRIOR = 16

# (C, npix): tests/test_mode_one_norm_gpu.py's GEOMETRY (every branch of bn_geometry), with the smallest legal pixel count first
GEOMETRY = [(4, 2), (4, 1023), (4, 4096), (4, 8195), (12, 2731), (260, 197), (64, 16401), (64, 16643), (64, 65791)]


def _layer(C, dev, seed, momentum=None, training=True):
    g = torch.Generator().manual_seed(seed)
    bn = BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.rand(C, generator=g) - 0.5)
        bn.running_mean.copy_(torch.randn(C, generator=g))
        bn.running_var.copy_(torch.rand(C, generator=g) * 2 + 0.2)
    bn.num_batches_tracked = bn.num_batches_tracked + PRIOR
    bn.momentum = momentum
    bn.acclimation_mode = True
    return bn.to(dev).train(training)


def _factor(momentum, bump, n_after):
    """the kernel's a as a double: the fp32 momentum, or fp32(1 / n) after the bump, or 0"""
    if momentum is not None:
        return float(torch.tensor(momentum, dtype=torch.float32))
    return float(torch.tensor(1.0 / n_after, dtype=torch.float32)) if bump else 0.0


def _batch64(x):
    xs = x.double().permute(1, 0, 2, 3).reshape(x.shape[1], -1)
    return xs.mean(1), xs.var(1, unbiased=True)


@torch.no_grad()
def _step64(bn_w, bn_b, eps, rm, rv, x, res, relu, a, batch=None):
    """one step in float64 from the running pair (rm, rv): batch mean, unbiased batch variance, updated pair, output"""
    mb, vu = batch if batch is not None else _batch64(x)
    rm2 = (1 - a) * rm.double() + a * mb
    rv2 = (1 - a) * rv.double() + a * vu
    scale = bn_w.double() / torch.sqrt(rv2 + eps)
    y = (x.double() - rm2.view(1, -1, 1, 1)) * scale.view(1, -1, 1, 1) + bn_b.double().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double()
    if relu:
        y = _relu_keeping_nan(y)
    return mb, vu, rm2, rv2, y


def _ratios(stats, rm_old, rv_old, y, ref):
    """error / bound of the four statistics rows (per channel) and the output's error over (1 + |y|)"""
    mb, vu, rm2, rv2, y64 = ref
    sd = vu.sqrt()
    tiny = 1e-300
    e_mb = (stats[0].double() - mb).abs() / (1e-5 * sd + 2.4e-7 * mb.abs() + tiny)
    e_vu = (stats[1].double() - vu).abs() / (1e-5 * vu + tiny)
    e_rm = (stats[2].double() - rm2).abs() / (1e-5 * sd + 2.4e-7 * torch.maximum(rm_old.double().abs(), mb.abs()) + tiny)
    e_rv = (stats[3].double() - rv2).abs() / (1e-5 * torch.maximum(rv_old.double(), vu) + tiny)
    e_y = (y.double() - y64).abs() / (1 + y64.abs())
    return e_mb, e_vu, e_rm, e_rv, e_y


def _call(bn, x, res, relu):
    stats = torch.full((4, x.shape[1]), float("nan"), dtype=torch.float32, device=x.device)
    y = bn._acclimate_hip_(x.clone(memory_format=torch.channels_last), res, relu, stats)
    return stats, y


@pytest.mark.parametrize("C,npix", GEOMETRY, ids=lambda v: str(v))
def test_entry_point_against_float64_across_the_launch_geometry(C, npix):
    dev = torch.device("cuda")
    x = _geometry_input(C, npix, dev, 7 * C + npix % 89)
    r = _activation(1, C, npix, 1, dev, 11 * C + npix % 83)
    batch = _batch64(x)
    combos = [(res_on, res_on, momentum, bump) for res_on in (False, True) for momentum in (0.1, None) for bump in (True, False)]
    combos += [(True, False, 0.1, True), (False, True, None, True)]
    for res_on, relu_on, momentum, bump in combos:
        what = "C %d, %d pixels, residual %d, relu %d, momentum %s, bump %d" % (C, npix, res_on, relu_on, momentum, bump)
        bn = _layer(C, dev, C + npix % 97, momentum, training=bump)
        rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
        ptrs = (bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.num_batches_tracked.data_ptr())
        res = r if res_on else None
        stats, y = _call(bn, x, res, relu_on)
        torch.cuda.synchronize()
        assert (bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.num_batches_tracked.data_ptr()) == ptrs
        assert int(bn.num_batches_tracked) == PRIOR + int(bump), what
        a = _factor(momentum, bump, PRIOR + 1)
        ref = _step64(bn.weight, bn.bias, bn.eps, rm0, rv0, x, res, relu_on, a, batch)
        e_mb, e_vu, e_rm, e_rv, e_y = _ratios(stats, rm0, rv0, y, ref)
        print("%s: error / bound: batch mean %.3f, batch variance %.3f, running mean %.3f, running variance %.3f; output error %.2e"
              % (what, float(e_mb.max()), float(e_vu.max()), float(e_rm.max()), float(e_rv.max()), float(e_y.max())))
        assert float(e_mb.max()) <= 1, (what, "batch mean", int(e_mb.argmax()))
        assert float(e_vu.max()) <= 1, (what, "batch variance", int(e_vu.argmax()))
        assert float(e_rm.max()) <= 1, (what, "running mean", int(e_rm.argmax()))
        assert float(e_rv.max()) <= 1, (what, "running variance", int(e_rv.argmax()))
        assert float(e_y.max()) <= 1e-4, (what, float(e_y.max()))
        assert torch.equal(stats[2], bn.running_mean) and torch.equal(stats[3], bn.running_var), what      # the buffers hold rm', rv'
        if momentum is None and not bump:
            assert torch.equal(bn.running_mean, rm0) and torch.equal(bn.running_var, rv0), what            # factor 0: unchanged bit for bit
        else:
            assert not torch.equal(bn.running_mean, rm0), what
        # a second run from the same initial state: the same bits everywhere
        with torch.no_grad():
            bn.running_mean.copy_(rm0)
            bn.running_var.copy_(rv0)
            bn.num_batches_tracked.fill_(PRIOR)
        stats2, y2 = _call(bn, x, res, relu_on)
        torch.cuda.synchronize()
        assert torch.equal(stats, stats2) and torch.equal(y, y2) and int(bn.num_batches_tracked) == PRIOR + int(bump), what
        assert torch.equal(stats2[2], bn.running_mean) and torch.equal(stats2[3], bn.running_var), what


@pytest.mark.parametrize("momentum", [None, 0.1], ids=["cumulative", "momentum0.1"])
def test_eight_steps_carry_the_state(momentum):
    """C = 64, 30 x 40, the input's mean drifting.  Every step against float64 started from the kernel's own previous state; the
    final state against an all-float64 run within 8 x the per-step bounds (each step contracts the error so far by 1 - a <= 1
    and adds at most one bound); the counter ends at prior + 8."""
    dev = torch.device("cuda")
    C, steps = 64, 8
    bn = _layer(C, dev, 21, momentum, training=True)
    rm64, rv64 = bn.running_mean.double(), bn.running_var.double()
    bound_rm = torch.zeros(C, dtype=torch.float64, device=dev)
    bound_rv = torch.zeros(C, dtype=torch.float64, device=dev)
    for k in range(steps):
        x = _activation(1, C, 30, 40, dev, 100 + k) + 0.3 * k
        rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
        stats, y = _call(bn, x, None, True)
        torch.cuda.synchronize()
        assert int(bn.num_batches_tracked) == PRIOR + k + 1
        a = _factor(momentum, True, PRIOR + k + 1)
        ref = _step64(bn.weight, bn.bias, bn.eps, rm0, rv0, x, None, True, a)
        e = _ratios(stats, rm0, rv0, y, ref)
        print("step %d: error / bound %s, output error %.2e" % (k, ["%.3f" % float(v.max()) for v in e[:4]], float(e[4].max())))
        assert all(float(v.max()) <= 1 for v in e[:4]) and float(e[4].max()) <= 1e-4, k
        assert torch.equal(stats[2], bn.running_mean) and torch.equal(stats[3], bn.running_var)
        mb, vu = ref[0], ref[1]
        bound_rm = torch.maximum(bound_rm, 1e-5 * vu.sqrt() + 2.4e-7 * torch.maximum(rm64.abs(), mb.abs()))
        bound_rv = torch.maximum(bound_rv, 1e-5 * torch.maximum(rv64, vu))
        rm64, rv64 = (1 - a) * rm64 + a * mb, (1 - a) * rv64 + a * vu
    e_rm = (bn.running_mean.double() - rm64).abs() / (8 * bound_rm)
    e_rv = (bn.running_var.double() - rv64).abs() / (8 * bound_rv)
    print("final state: error / (8 x bound): running mean %.3f, running variance %.3f" % (float(e_rm.max()), float(e_rv.max())))
    assert float(e_rm.max()) <= 1 and float(e_rv.max()) <= 1
    assert int(bn.num_batches_tracked) == PRIOR + steps


def test_one_pixel_is_refused_by_the_entry_point_and_raises_torchs_error_through_the_module():
    dev = torch.device("cuda")
    bn = _layer(8, dev, 2, 0.1, training=True)
    x = _activation(1, 8, 1, 1, dev, 3)
    l = _lib.lib()
    ws = torch.empty((l.dib_bn_mode_one_workspace_bytes(1, 8) // 4 + 1,), dtype=torch.float32, device=dev)
    rm0 = bn.running_mean.clone()
    rc = l.dib_bn_acclimate_nhwc(x.data_ptr(), None, 1, 8, bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(),
                                 bn.running_var.data_ptr(), bn.num_batches_tracked.data_ptr(), 1, 0.1, 1e-5, 0, ws.data_ptr(), ws.numel() * 4,
                                 None, _lib.stream_of(x))
    assert rc == _lib.DIB_EINVAL and b"more than one value per channel" in l.dib_last_error()
    torch.cuda.synchronize()
    assert torch.equal(bn.running_mean, rm0) and int(bn.num_batches_tracked) == PRIOR
    with torch.no_grad(), pytest.raises(ValueError, match="more than 1 value per channel"):
        bn(x)
    assert bn.last_path != "hip"


def test_entry_point_refusals_name_their_fault_and_launch_nothing():
    base, tensors, rows = refusal_case(torch.device("cuda"), bump=1, momentum=0.1)
    aligned = ALIGNED_16 + ", num_batches_dev 8-byte aligned"
    rows = [(what, change, code, aligned if fragment == ALIGNED_16 else fragment) for what, change, code, fragment in rows]
    E = _lib.DIB_EINVAL
    rows += [("one pixel", dict(n_pix=1), E, "more than one value per channel is needed to fold an unbiased variance in"),
             ("a bump without a counter", dict(num_batches_dev=None), E, "bump without num_batches_dev"),
             ("momentum 1.5", dict(momentum=1.5), E, "momentum above 1 (negative: cumulative average)"),
             ("momentum NaN", dict(momentum=float("nan")), E, "momentum above 1 (negative: cumulative average)"),
             ("counter + 4 bytes", dict(num_batches_dev=base["num_batches_dev"] + 4), E, aligned)]
    check_refusals("dib_bn_acclimate_nhwc", base, tensors, rows)
    assert tensors["counter"].tolist() == [PRIOR + 1, PRIOR]          # the accepted call at the end: its bump, and nothing beside it


def test_the_graph_decision_and_the_layer_agree_on_every_configuration():
    """C = 8, 3 x 5, no_grad: utils.acclimation_on_device (engine.evaluate: may the trunk be captured?) says yes exactly where the
    layer takes the HIP path on an input that path accepts.  Every combination of mode, track_running_stats, momentum, counter
    placement and affine, and three single departures from the plain layer; torch's own error on the torch path counts as torch."""
    dev = torch.device("cuda")
    x = _activation(1, 8, 3, 5, dev, 12)

    def noncontiguous_weight(bn):
        bn.weight = torch.nn.Parameter(torch.ones(16, device=dev)[::2])

    def float64_variance(bn):
        bn.running_var = bn.running_var.double()

    def switch_off(bn):
        backbone.FUSE_TEST_TIME_BN = False

    table = [(training, track, momentum, counter, affine, None) for training in (True, False) for track in (True, False)
             for momentum in (None, 0.1, 1.5) for counter in (("device", "host", None) if track else (None,)) for affine in (True, False)]
    table += [(True, True, None, "device", True, special) for special in (noncontiguous_weight, float64_variance, switch_off)]
    seen = set()
    old = backbone.FUSE_TEST_TIME_BN
    for training, track, momentum, counter, affine, special in table:
        what = "training %d, track %d, momentum %s, counter %s, affine %d, %s" % (training, track, momentum, counter, affine,
                                                                                  special.__name__ if special else "plain")
        bn = BatchNorm2d(8, momentum=momentum, affine=affine, track_running_stats=track).to(dev).train(training)
        bn.acclimation_mode = True
        if track and counter != "device":
            bn.num_batches_tracked = bn.num_batches_tracked.cpu() if counter == "host" else None
        try:
            if special:
                special(bn)
            model = torch.nn.Sequential(bn)
            with torch.no_grad():
                offered = utils.acclimation_on_device(model, dev)
                assert utils.acclimation_on_device(model, torch.device("cuda")) == offered, what
                try:
                    bn(x)
                    path = bn.last_path
                except _lib.DibError:
                    raise
                except Exception:
                    path = "torch"
        finally:
            backbone.FUSE_TEST_TIME_BN = old
        assert offered == (path == "hip") and path in ("hip", "torch"), (what, offered, path)
        seen.add(path)
    assert seen == {"hip", "torch"}


def test_a_nan_poisons_its_own_channel_only_and_passes_the_relu():
    """C = 8, 7 x 9, a single NaN in channel 5: its batch statistics, its running pair and its outputs are NaN, with the ReLU on and
    off; the other channels -- the three that share channel 5's float4 included -- stay within the bounds."""
    dev = torch.device("cuda")
    C = 8
    x = _activation(1, C, 7, 9, dev, 6)
    x[0, 5, 3, 4] = float("nan")
    r = _activation(1, C, 7, 9, dev, 8)
    others = [0, 1, 2, 3, 4, 6, 7]
    for res_on in (False, True):
        for relu_on in (False, True):
            bn = _layer(C, dev, 5, None, training=True)
            rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
            res = r if res_on else None
            stats, y = _call(bn, x, res, relu_on)
            torch.cuda.synchronize()
            ref = _step64(bn.weight, bn.bias, bn.eps, rm0, rv0, x, res, relu_on, _factor(None, True, PRIOR + 1))
            e = _ratios(stats, rm0, rv0, y, ref)
            assert all(float(v[others].max()) <= 1 for v in e[:4]) and float(e[4][:, others].max()) <= 1e-4
            assert bool(torch.isnan(stats[:, 5]).all()), stats[:, 5]
            assert bool(torch.isnan(bn.running_mean[5])) and bool(torch.isnan(bn.running_var[5]))
            assert bool(torch.isnan(y[:, 5]).all()), (relu_on, int(torch.isnan(y[:, 5]).sum()))
            assert not bool(torch.isnan(y[:, others]).any()) and not bool(torch.isnan(bn.running_mean[others]).any())
            assert int(bn.num_batches_tracked) == PRIOR + 1


def test_module_paths():
    """in place through the module's entry points; a training layer whose counter lives on the host takes the torch path"""
    dev = torch.device("cuda")
    bn = _layer(64, dev, 3, None, training=True)
    x = _activation(1, 64, 30, 40, dev, 4)
    ptr = bn.num_batches_tracked.data_ptr()
    with torch.no_grad():
        a = bn(x)
        assert bn.last_path == "hip" and int(bn.num_batches_tracked) == PRIOR + 1 and bn.num_batches_tracked.data_ptr() == ptr
        c = x.clone(memory_format=torch.channels_last)
        assert bn.forward_fused_(c, None, True) is c and bn.last_path == "hip" and int(bn.num_batches_tracked) == PRIOR + 2
        bn.num_batches_tracked = bn.num_batches_tracked.cpu()
        b = bn(x)
        assert bn.last_path == "torch" and int(bn.num_batches_tracked) == PRIOR + 3
        bn.eval()                                      # no bump: the counter is not read, wherever it lives
        bn(x)
        assert bn.last_path == "hip" and int(bn.num_batches_tracked) == PRIOR + 3
    assert a.shape == b.shape and a.data_ptr() != x.data_ptr()


# ---- the converted detector ----------------------------------------------------------------------------------------------------------

def _detector():
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    torch.manual_seed(0)
    m = fasterrcnn_resnet50_fpn(num_classes=91, pretrained=False, pretrained_backbone=False, min_size=128, max_size=160)
    g = torch.Generator().manual_seed(1)
    for mod in m.modules():
        if isinstance(mod, backbone.FrozenBatchNorm2d):
            C = mod.weight.shape[0]
            mod.weight.copy_(torch.rand(C, generator=g) + 0.5)
            mod.bias.copy_(torch.rand(C, generator=g) - 0.5)
            mod.running_mean.copy_(torch.rand(C, generator=g) - 0.5)
            mod.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    m = utils.convert_to_custom_batch_norm(m.to("cuda"), batch_norm_to_use=BatchNorm2d)
    m = utils.set_batch_norm_acclimation_mode(utils.set_batch_momentum_zero(utils.set_batch_norm_N(m, PRIOR)), True)
    return utils.turn_batch_norm_on(utils.copy_BN_stats_to_old(m).eval())


def test_converted_toy_trunk_runs_every_layer_on_the_hip_path_close_to_the_torch_path():
    fast = _detector()
    slow = copy.deepcopy(fast)
    with torch.no_grad():
        assert utils.acclimation_on_device(fast, torch.device("cuda"))
    g = torch.Generator().manual_seed(2)
    imgs = [(torch.rand((3, 128, 160), generator=g) * (0.5 + 0.25 * k)).cuda() for k in range(3)]
    fb = [(n, b) for n, b in fast.named_modules() if isinstance(b, BatchNorm2d)]
    sb = [(n, b) for n, b in slow.named_modules() if isinstance(b, BatchNorm2d)]
    assert len(fb) == len(sb) == 53
    seen = {}                                           # per layer of the torch path: the largest sigma_b^2 and |mean_b| it met

    def watch(name):
        def hook(mod, args):
            mb, vu = _batch64(args[0])
            old = seen.get(name)
            seen[name] = (mb.abs(), vu) if old is None else (torch.maximum(old[0], mb.abs()), torch.maximum(old[1], vu))
        return hook

    for n, b in sb:
        b.register_forward_pre_hook(watch(n))

    def features(m, img):
        with torch.no_grad():
            batch, _ = m.transform([img])
            return m.backbone(batch.tensors)

    for img in imgs:
        f = features(fast, img)
    assert [b.last_path for _, b in fb] == ["hip"] * 53
    old = backbone.FUSE_TEST_TIME_BN
    backbone.FUSE_TEST_TIME_BN = False
    try:
        with torch.no_grad():
            assert not utils.acclimation_on_device(slow, torch.device("cuda"))
        for img in imgs:
            s = features(slow, img)
    finally:
        backbone.FUSE_TEST_TIME_BN = old
    assert [b.last_path for _, b in sb] == ["torch"] * 53
    for k in f:
        rel = float((f[k] - s[k]).abs().max()) / float(s[k].abs().max())
        assert rel <= 1e-3, (k, rel)
    worst = [0.0, 0.0]
    for (n, a), (_, b) in zip(fb, sb):
        assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == PRIOR + 3 and a.num_batches_tracked.is_cuda
        mb, vu = seen[n]
        rm, rv = b.running_mean.double(), b.running_var.double()
        e_rm = (a.running_mean.double() - rm).abs() / (1e-5 * vu.sqrt() + 2.4e-7 * torch.maximum(rm.abs(), mb))
        e_rv = (a.running_var.double() - rv).abs() / (1e-5 * torch.maximum(rv, vu))
        worst = [max(worst[0], float(e_rm.max())), max(worst[1], float(e_rv.max()))]
        assert float(e_rm.max()) <= 1 and float(e_rv.max()) <= 1, (n, float(e_rm.max()), float(e_rv.max()))
    print("running buffers, HIP against torch path after 3 images: error / bound %.3f (mean), %.3f (variance)" % tuple(worst))


def graph_and_pipeline_child(out_path):
    from tests import _acclimate_children
    _acclimate_children.graph_and_pipeline(out_path)


def test_graphed_equals_eager_and_pipelined_equals_plain_bit_for_bit(tmp_path):
    from tests.test_ddp_gpu import _run_child
    r = _run_child(graph_and_pipeline_child, tmp_path)
    print(r)
    assert r["eager_paths"] == ["hip"] and r["eager_reproducible"] == [True, True]
    assert r["captured"] and r["detections"] > 0 and r["images_differ"]
    assert r["graphed_equals_eager"] == [True, True, True, True]
    assert r["counters"] == [PRIOR + 3]
    assert r["pipelined_captured"] and r["pipelined_images"] == 3 and r["pipelined_detections"] > 0
    assert r["pipelined_equals_plain"] == [True, True]
    assert r["pipelined_counters"] == [PRIOR + 3]
    assert r["syncs"]["acclimate"] == r["syncs"]["frozen"]          # the flag adds no synchronisation
    assert r["frozen_differs"]


# ---- driver ----------------------------------------------------------------------------------------------------------------------------

def evaluate_main_digest_child(out_path, argv):
    from tests import _gpu_children
    _gpu_children._guarded(_gpu_children._evaluate_main_digest, out_path, (argv,))


def test_two_runs_of_evaluate_main_acclimate_norm_print_identical_coco_stats(tmp_path):
    from tests.test_ddp_gpu import _run_child
    argv = ["--synthetic", "--synthetic_images", "3", "--acclimate_norm", "--blur_eval", "--gpu_blur", "--early_stop", "3"]
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    a = _run_child(evaluate_main_digest_child, tmp_path / "a", argv)
    b = _run_child(evaluate_main_digest_child, tmp_path / "b", argv)
    assert len(a["stat_lines"]) == 12 * 15
    assert a["stat_lines"] == b["stat_lines"]
    for cell in a["cells"]:
        assert a["cells"][cell] == b["cells"][cell], cell
