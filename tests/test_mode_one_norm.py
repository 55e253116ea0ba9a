"""`--mode_one_norm` (test-time batch-norm statistics, reference models/batchnorm.py:159-184, utils.py:59-77 / :122-135 /
:150-162, evaluate.py:234-237) without a GPU:

  * the torch path of models/batchnorm.BatchNorm2d equals the reference's own layer bit for bit (N = 1 and 2, odd H x W, planar
    and channels-last, zero-padded columns), and both equal tests/golden/bn_mode_one.npz;
  * the reference's three utils functions and this package's give the same converted detector and the same FPN outputs;
  * evaluate.main runs with --mode_one_norm (single model; ignored with --use_ensemble, as in the reference);
  * hipcc's resource report of csrc/dib_bnstats.hip shows no scratch.

`python tests/test_mode_one_norm.py --write` regenerates the fixture from the live reference."""
import contextlib
import copy
import importlib
import io
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ref_harness  # noqa: E402
from detectinblur_amd import utils  # noqa: E402
from detectinblur_amd.models import backbone  # noqa: E402
from detectinblur_amd.models.batchnorm import BatchNorm2d  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "bn_mode_one.npz")
N_TRACKED = 16
EPS = 1e-5

needs_reference = pytest.mark.skipif(not ref_harness.available(), reason="reference tree not present")


def _reference():
    ns = ref_harness.load()
    return ns, importlib.import_module("models.batchnorm")


# ---- fixture cases: (name, N, C, H, W, mean scale, std scale, zero columns) --------------------------------------------------------
CASES = [("n1_odd", 1, 8, 7, 9, 1.0, 1.0, 0),
         ("n2", 2, 12, 5, 6, 0.5, 2.0, 0),
         ("padded", 1, 16, 6, 13, 1.0, 1.0, 5),
         ("big_mean", 1, 8, 9, 11, 1000.0, 1.0, 0)]       # |mean| ~ 1e3 std: a sum-of-squares variance keeps no digit here


def _case_inputs(name, N, C, H, W, mscale, sscale, zcols, seed):
    rs = np.random.RandomState(seed)
    mean = (rs.uniform(-1, 1, C) * mscale).astype(np.float32)
    std = (rs.uniform(0.5, 1.5, C) * sscale).astype(np.float32)
    x = (mean[None, :, None, None] + std[None, :, None, None] * rs.standard_normal((N, C, H, W))).astype(np.float32)
    if zcols:
        x[..., W - zcols:] = 0.0                  # batch_images' zero padding: part of the statistics, as in the reference
    rm = (mean + rs.uniform(-0.3, 0.3, C) * mscale).astype(np.float32)
    rv = (std * std * rs.uniform(0.7, 1.3, C)).astype(np.float32)
    w = rs.uniform(0.5, 1.5, C).astype(np.float32)
    b = rs.uniform(-0.5, 0.5, C).astype(np.float32)
    return dict(x=x, running_mean=rm, running_var=rv, weight=w, bias=b)


def restate64(x, running_mean, running_var, weight, bias, n=N_TRACKED, eps=EPS):
    """float64 restatement: the mixed statistics and the normalised output."""
    x = np.asarray(x, np.float64)
    C = x.shape[1]
    xs = np.moveaxis(x, 1, 0).reshape(C, -1)
    mb, vb = xs.mean(1), xs.var(1)
    f, g = n / (n + 1.0), 1.0 / (n + 1.0)
    mean = f * np.asarray(running_mean, np.float64) + g * mb
    var = f * np.asarray(running_var, np.float64) + g * vb
    scale = np.asarray(weight, np.float64) / np.sqrt(var + eps)
    y = (x - mean[None, :, None, None]) * scale[None, :, None, None] + np.asarray(bias, np.float64)[None, :, None, None]
    return mean, var, y


def _layer(cls, d, channels_last=False):
    C = d["running_mean"].shape[0]
    bn = cls(C)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(d["weight"]))
        bn.bias.copy_(torch.from_numpy(d["bias"]))
        bn.running_mean.copy_(torch.from_numpy(d["running_mean"]))
        bn.running_var.copy_(torch.from_numpy(d["running_var"]))
    bn.num_batches_tracked = bn.num_batches_tracked + N_TRACKED
    bn.mode_one = True
    bn.eval()
    return bn


def _x(d, channels_last):
    x = torch.from_numpy(d["x"])
    return x.contiguous(memory_format=torch.channels_last) if channels_last else x


def build_fixture():
    _, RB = _reference()
    out = {}
    for k, (name, *shape) in enumerate(CASES):
        d = _case_inputs(name, *shape, seed=100 + k)
        with torch.no_grad():
            y = _layer(RB.BatchNorm2d, d)(_x(d, False))
        mean64, var64, y64 = restate64(**d)
        for key, v in d.items():
            out["%s/%s" % (name, key)] = v
        out[name + "/y_ref"] = y.numpy()
        out[name + "/mean64"], out[name + "/var64"], out[name + "/y64"] = mean64, var64, y64
    out["num_batches_tracked"] = np.int64(N_TRACKED)
    out["eps"] = np.float32(EPS)
    return out


def load_fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def fixture_case(fx, name):
    return {k: fx["%s/%s" % (name, k)] for k in ("x", "running_mean", "running_var", "weight", "bias")}


# ---- layer level -----------------------------------------------------------------------------------------------------------------

def _layer_cases():
    rs = np.random.RandomState(7)
    out = []
    for N, C, H, W, zc in ((1, 8, 7, 9, 0), (2, 12, 5, 6, 0), (1, 16, 6, 13, 5), (2, 4, 3, 11, 4), (1, 64, 16, 24, 0)):
        for cl in (False, True):
            d = _case_inputs("", N, C, H, W, rs.uniform(0.1, 3.0), rs.uniform(0.5, 2.0), zc, int(rs.randint(1 << 30)))
            out.append(pytest.param(d, cl, id="N%d_C%d_%dx%d%s_%s" % (N, C, H, W, "_pad%d" % zc if zc else "", "nhwc" if cl else "nchw")))
    return out


@needs_reference
@pytest.mark.parametrize("d, channels_last", _layer_cases())
def test_torch_path_equals_the_reference_layer_bit_for_bit(d, channels_last):
    _, RB = _reference()
    ref, ours = _layer(RB.BatchNorm2d, d), _layer(BatchNorm2d, d)
    with torch.no_grad():
        want = ref(_x(d, channels_last))
        got = ours(_x(d, channels_last))
    assert ours.last_path == "torch"
    assert torch.equal(got, want)


def test_mode_one_off_is_torch_batch_norm():
    rs = np.random.RandomState(3)
    d = _case_inputs("", 2, 8, 5, 7, 1.0, 1.0, 0, 3)
    ours = _layer(BatchNorm2d, d)
    ours.mode_one = False
    plain = torch.nn.BatchNorm2d(8)
    plain.load_state_dict(ours.state_dict())
    for train in (False, True):
        ours.train(train)
        plain.train(train)
        x = torch.from_numpy(rs.standard_normal((2, 8, 5, 7)).astype(np.float32))
        with torch.no_grad():
            assert torch.equal(ours(x), plain(x))
        assert torch.equal(ours.running_mean, plain.running_mean) and torch.equal(ours.num_batches_tracked, plain.num_batches_tracked)


def test_fixture_holds_the_float64_restatement_and_the_torch_path_reproduces_it():
    fx = load_fixture()
    assert os.path.getsize(GOLDEN) < 256 * 1024
    assert int(fx["num_batches_tracked"]) == N_TRACKED
    for name, *_ in CASES:
        d = fixture_case(fx, name)
        mean64, var64, y64 = restate64(**d)
        assert np.array_equal(mean64, fx[name + "/mean64"]) and np.array_equal(var64, fx[name + "/var64"])
        assert np.array_equal(y64, fx[name + "/y64"])
        with torch.no_grad():
            y = _layer(BatchNorm2d, d)(_x(d, False)).numpy()
        assert np.array_equal(y, fx[name + "/y_ref"]), name
        assert np.all(np.abs(y - y64) <= 1e-4 * (1 + np.abs(y64))), name


@needs_reference
def test_fixture_matches_the_live_reference():
    want = build_fixture()
    got = load_fixture()
    assert sorted(want) == sorted(got)
    for k in want:
        assert np.array_equal(np.asarray(want[k]), got[k]), k


# ---- model level -----------------------------------------------------------------------------------------------------------------

def _detector():
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    torch.manual_seed(0)
    m = fasterrcnn_resnet50_fpn(num_classes=91, pretrained=False, pretrained_backbone=False, min_size=128, max_size=160)
    g = torch.Generator().manual_seed(1)
    for mod in m.modules():
        if isinstance(mod, backbone.FrozenBatchNorm2d):        # non-trivial statistics, so that the conversion has something to keep
            C = mod.weight.shape[0]
            mod.weight.copy_(torch.rand(C, generator=g) + 0.5)
            mod.bias.copy_(torch.rand(C, generator=g) - 0.5)
            mod.running_mean.copy_(torch.rand(C, generator=g) - 0.5)
            mod.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    return m.eval()


def _bns(model, cls):
    return [(n, m) for n, m in model.named_modules() if isinstance(m, cls)]


@needs_reference
def test_reference_utils_and_ours_convert_the_detector_identically():
    ns, RB = _reference()
    ns.utils.torchvision.ops.misc.FrozenBatchNorm2d = backbone.FrozenBatchNorm2d      # the reference's isinstance target
    base = _detector()
    ref = copy.deepcopy(base)
    ref = ns.utils.convert_to_custom_batch_norm(ref, batch_norm_to_use=RB.BatchNorm2d)
    ref = ns.utils.set_batch_norm_N(ref, 16)
    ref = ns.utils.set_batch_norm_mode1(ref, True)
    ours = copy.deepcopy(base)
    ours = utils.convert_to_custom_batch_norm(ours, batch_norm_to_use=BatchNorm2d)
    ours = utils.set_batch_norm_N(ours, 16)
    ours = utils.set_batch_norm_mode1(ours, True)
    rb, ob = _bns(ref, RB.BatchNorm2d), _bns(ours, BatchNorm2d)
    assert len(rb) == len(ob) == 53
    assert not _bns(ours, backbone.FrozenBatchNorm2d)
    for (rn, r), (on, o) in zip(rb, ob):
        assert rn == on
        assert r.eps == o.eps == 1e-5 and r.mode_one and o.mode_one
        assert int(r.num_batches_tracked) == int(o.num_batches_tracked) == 16
        assert o.num_batches_tracked.dtype == torch.int64
        assert isinstance(o.weight, torch.nn.Parameter) and isinstance(o.bias, torch.nn.Parameter)
        for k in ("weight", "bias", "running_mean", "running_var"):
            assert torch.equal(getattr(r, k), getattr(o, k)), (rn, k)
    x = torch.Generator().manual_seed(5)
    img = torch.rand((1, 3, 128, 160), generator=x).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        fr, fo = ref.backbone(img), ours.backbone(img)
        ff = base.backbone(img)
    assert all(m.last_path == "torch" for _, m in ob)
    for k in fo:
        assert torch.equal(fr[k], fo[k]), k
    assert max(float((fo[k] - ff[k]).abs().max()) for k in fo) > 1e-3        # the remedy changes the network


def test_conversion_drops_the_cached_trunk_state():
    m = _detector()
    m.__dict__["_trunk_graphs"] = object()
    m.__dict__["_trunk_ptrs"] = (1, 2)
    m.backbone.__dict__["_dib_fold_pairs"] = []
    m.backbone.__dict__["_dib_fold_state"] = (0, 0)
    utils.convert_to_custom_batch_norm(m, batch_norm_to_use=BatchNorm2d)
    assert "_trunk_graphs" not in m.__dict__ and "_trunk_ptrs" not in m.__dict__
    assert "_dib_fold_pairs" not in m.backbone.__dict__ and "_dib_fold_state" not in m.backbone.__dict__
    bn = m.backbone.body.bn1
    assert isinstance(bn, BatchNorm2d) and bn.num_batches_tracked.device == bn.running_mean.device


# ---- driver --------------------------------------------------------------------------------------------------------------------------

_ARGV = ["--synthetic", "--synthetic_size", "128", "160", "--min_size", "128", "--max_size", "160", "--device", "cpu", "--mode_one_norm",
         "--vanilla_eval", "--early_stop", "1"]


def _run_main(argv):
    from detectinblur_amd import evaluate
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = evaluate.main(evaluate.build_parser().parse_args(argv))
    return res, buf.getvalue()


def test_evaluate_main_runs_with_mode_one_norm_on_cpu():
    res, out = _run_main(_ARGV)
    ce = res["Clean"]
    assert len(ce.coco_eval["bbox"].stats) == 12
    assert "ignored" not in out


class _FirstCell(Exception):
    pass


def _first_sweep_cell(argv, monkeypatch):
    """evaluate.main up to the end of the sweep's first cell: that cell's result and the ensemble it ran."""
    from detectinblur_amd import evaluate
    seen = {}

    def first(*a, **k):
        seen["result"] = real(*a, **k)
        seen["ensemble"] = k.get("ensemble_models")
        raise _FirstCell()

    real = evaluate.evaluate
    monkeypatch.setattr(evaluate, "evaluate", first)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(_FirstCell):
        evaluate.main(evaluate.build_parser().parse_args(argv))
    monkeypatch.setattr(evaluate, "evaluate", real)
    return seen, buf.getvalue()


def test_mode_one_norm_is_ignored_with_the_ensemble(monkeypatch):
    # the ensemble routes by blur: a sweep cell (CPU blur), not --vanilla_eval
    argv = [a for a in _ARGV if a != "--vanilla_eval"] + ["--use_ensemble", "--blur_eval", "--cpu_blur"]
    on, out = _first_sweep_cell(argv, monkeypatch)
    assert "--mode_one_norm is ignored with --use_ensemble" in out
    off, _ = _first_sweep_cell([a for a in argv if a != "--mode_one_norm"], monkeypatch)
    assert len(on["ensemble"]) == 4
    for m in on["ensemble"]:
        assert not _bns(m, BatchNorm2d) and len(_bns(m, backbone.FrozenBatchNorm2d)) == 53
    a, b = on["result"], off["result"]
    assert sorted(a["detections"]) == sorted(b["detections"]) and len(a["detections"]) >= 1
    for k in a["detections"]:
        for f in ("boxes", "scores", "labels"):
            assert torch.equal(a["detections"][k][f], b["detections"][k][f])
    assert list(a.coco_eval["bbox"].stats) == list(b.coco_eval["bbox"].stats)


def test_unfrozen_batch_norm_stays_refused():
    from detectinblur_amd import train as TR
    a = TR.build_parser().parse_args(["--unfrozen_batch_norm"])
    with pytest.raises(SystemExit, match="outside the built hot path"):
        TR.reject_out_of_scope(a)


# ---- kernel resources ----------------------------------------------------------------------------------------------------------------

def test_mode_one_kernels_use_no_scratch():
    from tests._kernel_resources import kernel_resources
    out = kernel_resources("dib_bnstats.hip")
    for frag in ("bn_partial_kernel", "bn_finalize_kernel", "bn_apply_kernel"):
        names = [n for n in out if frag in n]
        assert names, frag
        for n in names:
            assert out[n]["ScratchSize"] == 0, (n, out[n])
            assert out[n]["Occupancy"] >= 4, (n, out[n])


if __name__ == "__main__":
    if "--write" in sys.argv:
        np.savez_compressed(GOLDEN, **build_fixture())
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
