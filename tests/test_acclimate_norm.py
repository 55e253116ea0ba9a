"""`--acclimate_norm` (online batch-norm statistics: the reference layer's `acclimation_mode`, models/batchnorm.py:142-157, and
the helpers of its utils.py:80-120 / :136-148 / :193-217) without a GPU:

  * the torch path of models/batchnorm.BatchNorm2d equals the reference's own layer bit for bit over 3-step sequences -- outputs,
    both running buffers and the counter; momentum 0.1 / None x training / eval mode; N = 1 and 2, odd H x W, planar and
    channels-last -- and both equal tests/golden/bn_acclimation.npz;
  * the ported helpers and the reference's leave identical converted detectors; restore_BN_stats_from_old keeps every address;
  * the driver's defaults and refusals; engine.evaluate on the CPU device: counters, passes from the snapshot, carry-over;
    a pass without the flag leaves the state_dict alone;
  * hipcc's resource report of csrc/dib_bnstats.hip shows no scratch in any kernel.

`python tests/test_acclimate_norm.py --write` regenerates the fixture from the live reference."""
import contextlib
import copy
import importlib
import io
import os
import re
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "bn_acclimation.npz")
PRIOR = 16
STEPS = 3

needs_reference = pytest.mark.skipif(not ref_harness.available(), reason="reference tree not present")


_REFERENCE = {}


def _reference():
    """The reference's modules (utils, models.batchnorm), loaded once and without leaking into later test files: ref_harness.load()
    installs stub modules (torchvision, torch.utils.tensorboard, cv2, ...), the reference's top-level modules and its directory on
    sys.path; all of that is put back right after loading (as tests/test_augmix.py does), the handles kept here stay usable."""
    if not _REFERENCE:
        from unittest import mock
        modules, path, np_math, loaded = dict(sys.modules), list(sys.path), hasattr(np, "math"), dict(ref_harness._loaded)
        root = os.path.realpath(ref_harness.REFERENCE_ROOT)

        def foreign(mod):
            if isinstance(mod, mock.MagicMock) or getattr(mod, "__name__", None) == "cv2":
                return True
            places = [getattr(mod, "__file__", None) or ""] + list(getattr(mod, "__path__", None) or [])
            return any(str(p).startswith(root) for p in places)

        try:
            _REFERENCE["ns"] = ref_harness.load()
            _REFERENCE["batchnorm"] = importlib.import_module("models.batchnorm")
        finally:
            for name in [k for k in sys.modules if k not in modules or sys.modules[k] is not modules[k]]:
                if foreign(sys.modules[name]):
                    del sys.modules[name]
            sys.modules.update({k: v for k, v in modules.items() if k not in sys.modules})
            ref_harness._loaded.clear()
            ref_harness._loaded.update(loaded)
            if not np_math and hasattr(np, "math"):
                del np.math
            sys.path[:] = path
    return _REFERENCE["ns"], _REFERENCE["batchnorm"]


# ---- sequences ---------------------------------------------------------------------------------------------------------------------

CONFIGS = [(0.1, True), (0.1, False), (None, True), (None, False)]          # (momentum, training mode)
SHAPES = [(1, 8, 7, 9), (2, 12, 5, 7)]                                      # N, C, odd H x W
FIXTURE_SHAPES = [(1, 8, 5, 7), (2, 4, 3, 5)]                               # the committed sequences: a few tens of KB


def _sequence(N, C, H, W, seed):
    """initial layer state and STEPS inputs whose mean drifts away from the running mean"""
    rs = np.random.RandomState(seed)
    mean = rs.uniform(-1, 1, C).astype(np.float32)
    std = rs.uniform(0.5, 1.5, C).astype(np.float32)
    xs = [(mean[None, :, None, None] + 0.4 * k + std[None, :, None, None] * rs.standard_normal((N, C, H, W))).astype(np.float32)
          for k in range(STEPS)]
    return dict(x=np.stack(xs), running_mean=(mean + rs.uniform(-0.3, 0.3, C)).astype(np.float32),
                running_var=(std * std * rs.uniform(0.7, 1.3, C)).astype(np.float32),
                weight=rs.uniform(0.5, 1.5, C).astype(np.float32), bias=rs.uniform(-0.5, 0.5, C).astype(np.float32))


def _layer(cls, d, momentum, training):
    bn = cls(d["running_mean"].shape[0])
    with torch.no_grad():
        for k in ("weight", "bias", "running_mean", "running_var"):
            getattr(bn, k).copy_(torch.from_numpy(d[k]))
    bn.num_batches_tracked = bn.num_batches_tracked + PRIOR
    bn.momentum = momentum
    bn.acclimation_mode = True
    return bn.train(training)


def _run(bn, d, channels_last):
    """per step: output, running_mean, running_var, counter"""
    out = []
    for k in range(STEPS):
        x = torch.from_numpy(d["x"][k])
        if channels_last:
            x = x.contiguous(memory_format=torch.channels_last)
        with torch.no_grad():
            y = bn(x)
        out.append((y.clone(), bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)))
    return out


def _sequence_cases():
    out = []
    for si, shape in enumerate(SHAPES):
        for ci, (momentum, training) in enumerate(CONFIGS):
            for cl in (False, True):
                out.append(pytest.param(shape, momentum, training, cl, 50 + 4 * si + ci,
                                        id="N%d_C%d_%dx%d_m%s_%s_%s" % (*shape, momentum, "train" if training else "eval", "nhwc" if cl else "nchw")))
    return out


@needs_reference
@pytest.mark.parametrize("shape, momentum, training, channels_last, seed", _sequence_cases())
def test_torch_path_equals_the_reference_layer_bit_for_bit(shape, momentum, training, channels_last, seed):
    _, RB = _reference()
    d = _sequence(*shape, seed=seed)
    ours = _layer(BatchNorm2d, d, momentum, training)
    want = _run(_layer(RB.BatchNorm2d, d, momentum, training), d, channels_last)
    got = _run(ours, d, channels_last)
    assert ours.last_path == "torch"
    for k, (w, g) in enumerate(zip(want, got)):
        assert torch.equal(g[0], w[0]), ("output", k)
        assert torch.equal(g[1], w[1]) and torch.equal(g[2], w[2]), ("running statistics", k)
        assert g[3] == w[3] == PRIOR + ((k + 1) if training else 0), ("counter", k)
    if momentum is None and not training:
        assert torch.equal(got[-1][1], torch.from_numpy(d["running_mean"]))      # factor 0.0: nothing moves
    else:
        assert not torch.equal(got[-1][1], torch.from_numpy(d["running_mean"]))


def test_acclimation_wins_over_mode_one_and_both_off_is_torch_batch_norm():
    d = _sequence(1, 8, 7, 9, seed=3)
    a, b = _layer(BatchNorm2d, d, None, True), _layer(BatchNorm2d, d, None, True)
    b.mode_one = True
    for (ya, *sa), (yb, *sb) in zip(_run(a, d, False), _run(b, d, False)):
        assert torch.equal(ya, yb) and all(torch.equal(torch.as_tensor(p), torch.as_tensor(q)) for p, q in zip(sa, sb))
    off = _layer(BatchNorm2d, d, 0.1, False)
    off.acclimation_mode = False
    plain = torch.nn.BatchNorm2d(8).eval()
    plain.load_state_dict(off.state_dict())
    x = torch.from_numpy(d["x"][0])
    with torch.no_grad():
        assert torch.equal(off(x), plain(x))


def test_one_value_per_channel_raises_torchs_error():
    d = _sequence(1, 8, 1, 1, seed=4)
    bn = _layer(BatchNorm2d, d, 0.1, True)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        bn(torch.from_numpy(d["x"][0]))


# ---- fixture -------------------------------------------------------------------------------------------------------------------------

def _fixture_cases():
    return [("%s_m%s_%s" % ("n%d" % shape[0], momentum, "train" if training else "eval"), shape, momentum, training, 200 + 4 * si + ci)
            for si, shape in enumerate(FIXTURE_SHAPES) for ci, (momentum, training) in enumerate(CONFIGS)]


def build_fixture():
    _, RB = _reference()
    out = {}
    for name, shape, momentum, training, seed in _fixture_cases():
        d = _sequence(*shape, seed=seed)
        steps = _run(_layer(RB.BatchNorm2d, d, momentum, training), d, False)
        for key, v in d.items():
            out["%s/%s" % (name, key)] = v
        out[name + "/y_ref"] = np.stack([s[0].numpy() for s in steps])
        out[name + "/running_mean_ref"] = np.stack([s[1].numpy() for s in steps])
        out[name + "/running_var_ref"] = np.stack([s[2].numpy() for s in steps])
        out[name + "/counter_ref"] = np.asarray([s[3] for s in steps], np.int64)
    out["num_batches_tracked"] = np.int64(PRIOR)
    return out


def load_fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def restate64(x, rm, rv, weight, bias, a, eps=1e-5):
    """float64 restatement of one step: batch mean, unbiased batch variance, the updated running pair and the output"""
    x = np.asarray(x, np.float64)
    C = x.shape[1]
    xs = np.moveaxis(x, 1, 0).reshape(C, -1)
    mb, vu = xs.mean(1), xs.var(1, ddof=1)
    rm2 = (1 - a) * np.asarray(rm, np.float64) + a * mb
    rv2 = (1 - a) * np.asarray(rv, np.float64) + a * vu
    scale = np.asarray(weight, np.float64) / np.sqrt(rv2 + eps)
    y = (x - rm2[None, :, None, None]) * scale[None, :, None, None] + np.asarray(bias, np.float64)[None, :, None, None]
    return mb, vu, rm2, rv2, y


def test_fixture_is_reproduced_by_the_torch_path_and_close_to_float64():
    fx = load_fixture()
    assert os.path.getsize(GOLDEN) < 256 * 1024
    assert int(fx["num_batches_tracked"]) == PRIOR
    for name, shape, momentum, training, seed in _fixture_cases():
        d = {k: fx["%s/%s" % (name, k)] for k in ("x", "running_mean", "running_var", "weight", "bias")}
        want = _sequence(*shape, seed=seed)
        assert all(np.array_equal(d[k], want[k]) for k in d), name
        got = _run(_layer(BatchNorm2d, d, momentum, training), d, False)
        rm, rv = d["running_mean"].astype(np.float64), d["running_var"].astype(np.float64)
        for k, (y, m, v, n) in enumerate(got):
            assert np.array_equal(y.numpy(), fx[name + "/y_ref"][k]), (name, k)
            assert np.array_equal(m.numpy(), fx[name + "/running_mean_ref"][k]), (name, k)
            assert np.array_equal(v.numpy(), fx[name + "/running_var_ref"][k]), (name, k)
            assert n == int(fx[name + "/counter_ref"][k]) == PRIOR + ((k + 1) if training else 0), (name, k)
            a = momentum if momentum is not None else (1.0 / n if training else 0.0)
            mb, vu, rm, rv, y64 = restate64(d["x"][k], rm, rv, d["weight"], d["bias"], a)
            assert np.all(np.abs(m.numpy() - rm) <= 1e-5 * np.sqrt(vu) + 2.4e-7 * np.maximum(np.abs(rm), np.abs(mb))), (name, k)
            assert np.all(np.abs(v.numpy() - rv) <= 1e-5 * np.maximum(rv, vu)), (name, k)
            assert np.all(np.abs(y.numpy() - y64) <= 1e-4 * (1 + np.abs(y64))), (name, k)


@needs_reference
def test_fixture_matches_the_live_reference():
    want, got = build_fixture(), load_fixture()
    assert sorted(want) == sorted(got)
    for k in want:
        assert np.array_equal(np.asarray(want[k]), got[k]), k


# ---- helpers -------------------------------------------------------------------------------------------------------------------------

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
    return m.eval()


def _bns(model, cls):
    return [(n, m) for n, m in model.named_modules() if isinstance(m, cls)]


def _arm(U, m, cls):
    """the driver's sequence (evaluate.py), through either module's helpers"""
    m = U.convert_to_custom_batch_norm(m, batch_norm_to_use=cls)
    m = U.set_batch_norm_N(m, PRIOR)
    m = U.set_batch_momentum_zero(m)
    m = U.set_batch_norm_acclimation_mode(m, True)
    return U.copy_BN_stats_to_old(m)


@needs_reference
def test_ported_helpers_and_the_references_leave_identical_detectors():
    ns, RB = _reference()
    ns.utils.torchvision.ops.misc.FrozenBatchNorm2d = backbone.FrozenBatchNorm2d      # the reference's isinstance target
    base = _detector()
    ref, ours = _arm(ns.utils, copy.deepcopy(base), RB.BatchNorm2d), _arm(utils, copy.deepcopy(base), BatchNorm2d)

    def same(what):
        rb, ob = _bns(ref, RB.BatchNorm2d), _bns(ours, BatchNorm2d)
        assert len(rb) == len(ob) == 53
        for (rn, r), (on, o) in zip(rb, ob):
            assert rn == on
            assert r.training == o.training and r.momentum == o.momentum and r.acclimation_mode == o.acclimation_mode, (what, rn)
            for k in ("running_mean", "running_var", "num_batches_tracked", "old_running_mean", "old_running_var", "old_num_batches_tracked"):
                assert torch.equal(getattr(r, k), getattr(o, k)), (what, rn, k)
        return ob

    ob = same("armed")
    assert all(o.acclimation_mode and o.momentum is None and int(o.old_num_batches_tracked) == PRIOR for _, o in ob)
    ref.eval(), ours.eval()
    ref, ours = ns.utils.turn_batch_norm_on(ref), utils.turn_batch_norm_on(ours)
    ob = same("on")
    assert all(o.training for _, o in ob) and not ours.training and not ours.backbone.training
    ref, ours = ns.utils.set_batch_momentum(ref, 0.05), utils.set_batch_momentum(ours, 0.05)
    assert all(o.momentum == 0.05 for _, o in same("momentum"))
    ref, ours = ns.utils.reset_batch_norm_values(ref), utils.reset_batch_norm_values(ours)
    ob = same("reset")
    assert all(int(o.num_batches_tracked) == 0 and float(o.running_var.min()) == 1.0 and int(o.old_num_batches_tracked) == PRIOR for _, o in ob)
    ref, ours = ns.utils.set_batch_norm_acclimation_mode(ref, False), utils.set_batch_norm_acclimation_mode(ours, False)
    assert not any(o.acclimation_mode for _, o in same("off"))


def test_snapshot_stays_out_of_the_state_dict_and_restore_keeps_every_address():
    m = _detector()
    keys = None
    m = utils.convert_to_custom_batch_norm(m, batch_norm_to_use=BatchNorm2d)
    keys = sorted(m.state_dict())
    m = _arm(utils, m, BatchNorm2d)
    assert sorted(m.state_dict()) == keys
    bns = [b for _, b in _bns(m, BatchNorm2d)]
    before = [(b.running_mean.data_ptr(), b.running_var.data_ptr(), b.num_batches_tracked.data_ptr()) for b in bns]
    want = [(b.running_mean.clone(), b.running_var.clone(), b.num_batches_tracked.clone()) for b in bns]
    for b in bns:
        with torch.no_grad():
            b.running_mean.add_(1.0)
            b.running_var.mul_(2.0)
            b.num_batches_tracked.add_(5)
    m.__dict__["_trunk_graphs"] = marker = object()
    assert utils.restore_BN_stats_from_old(m) is m
    assert m.__dict__["_trunk_graphs"] is marker                    # captured trunks stay: the addresses have not moved
    assert [(b.running_mean.data_ptr(), b.running_var.data_ptr(), b.num_batches_tracked.data_ptr()) for b in bns] == before
    for b, (rm, rv, n) in zip(bns, want):
        assert torch.equal(b.running_mean, rm) and torch.equal(b.running_var, rv) and torch.equal(b.num_batches_tracked, n)
        assert b.num_batches_tracked.dtype == torch.int64
    with pytest.raises(RuntimeError, match="no snapshot"):
        utils.restore_BN_stats_from_old(utils.convert_to_custom_batch_norm(_detector(), batch_norm_to_use=BatchNorm2d))


def test_state_on_the_cpu_is_never_offered_to_a_graph():
    m = _arm(utils, _detector(), BatchNorm2d)
    assert utils.acclimation_on_device(_detector(), torch.device("cpu"))          # nothing acclimates: nothing to decide
    assert not utils.acclimation_on_device(m, torch.device("cpu"))
    assert not utils.acclimation_on_device(m, torch.device("cuda"))               # the buffers are CPU tensors


# ---- driver ----------------------------------------------------------------------------------------------------------------------------

_ARGV = ["--synthetic", "--synthetic_images", "2", "--synthetic_size", "128", "160", "--min_size", "128", "--max_size", "160", "--device", "cpu",
         "--vanilla_eval"]


def test_parser_defaults():
    from detectinblur_amd import evaluate
    a = evaluate.build_parser().parse_args([])
    assert a.acclimate_norm is False and a.acclimation_momentum is None and a.acclimation_prior is None and a.acclimation_carry_over is False
    assert evaluate.ACCLIMATION_PRIOR == 16
    a = evaluate.build_parser().parse_args(["--acclimate_norm", "--acclimation_momentum", "0.05", "--acclimation_prior", "4", "--acclimation_carry_over"])
    assert a.acclimate_norm and a.acclimation_momentum == 0.05 and a.acclimation_prior == 4 and a.acclimation_carry_over


@pytest.mark.parametrize("extra, message", [
    (["--acclimate_norm", "--mode_one_norm"], "--acclimate_norm with --mode_one_norm"),
    (["--acclimate_norm", "--use_ensemble"], "--acclimate_norm with --use_ensemble"),
    (["--acclimate_norm", "--amp"], "--amp with --acclimate_norm"),
    (["--acclimation_momentum", "0.1"], "--acclimation_momentum needs --acclimate_norm"),
    (["--acclimation_prior", "16"], "--acclimation_prior needs --acclimate_norm"),
    (["--acclimation_carry_over"], "--acclimation_carry_over needs --acclimate_norm"),
], ids=lambda v: "_".join(v).replace("--", "") if isinstance(v, list) else None)
def test_refusals_at_start(extra, message, monkeypatch):
    from detectinblur_amd import evaluate
    monkeypatch.setattr(evaluate, "fasterrcnn_resnet50_fpn", lambda *a, **k: pytest.fail("a detector was built"))
    with pytest.raises(SystemExit, match=re.escape(message)):
        evaluate.main(evaluate.build_parser().parse_args(_ARGV + extra))


def _passes(argv, monkeypatch, passes):
    """evaluate.main with engine.evaluate called `passes` times on the model and loader the driver built: the model, per pass
    the result, and the batch-norm state before the first and after every pass"""
    from detectinblur_amd import evaluate
    seen = {"results": [], "states": []}
    real = evaluate.evaluate

    def state(model):
        return {k: v.clone() for k, v in model.state_dict().items()}

    def several(model, loader, **kw):
        seen["model"] = model
        seen["states"].append(state(model))
        for _ in range(passes):
            seen["results"].append(real(model, loader, **kw))
            seen["states"].append(state(model))
        return seen["results"][-1]

    monkeypatch.setattr(evaluate, "evaluate", several)
    with contextlib.redirect_stdout(io.StringIO()):
        evaluate.main(evaluate.build_parser().parse_args(argv))
    monkeypatch.setattr(evaluate, "evaluate", real)
    return seen


def _same_detections(a, b):
    assert sorted(a["detections"]) == sorted(b["detections"]) and len(a["detections"]) == 2
    for k in a["detections"]:
        for f in ("boxes", "scores", "labels"):
            assert torch.equal(a["detections"][k][f], b["detections"][k][f]), (k, f)


def _counters(state):
    return sorted({int(v) for k, v in state.items() if k.endswith("num_batches_tracked")})


def test_engine_passes_start_from_the_snapshot_and_count_the_images(monkeypatch):
    seen = _passes(_ARGV + ["--acclimate_norm"], monkeypatch, passes=2)
    bns = _bns(seen["model"], BatchNorm2d)
    assert len(bns) == 53 and all(b.acclimation_mode and b.momentum is None and b.training and b.last_path == "torch" for _, b in bns)
    assert not seen["model"].training
    s0, s1, s2 = seen["states"]
    assert _counters(s0) == [16] and _counters(s1) == [18] and _counters(s2) == [18]          # prior + the pass's two images
    assert all(torch.equal(s1[k], s2[k]) for k in s1)                                          # identical final statistics
    moved = [k for k in s0 if not torch.equal(s0[k], s1[k])]
    assert len(moved) == 3 * 53 and all(k.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked") for k in moved)
    _same_detections(*seen["results"])


def test_carry_over_runs_the_statistics_on_through_the_passes(monkeypatch):
    seen = _passes(_ARGV + ["--acclimate_norm", "--acclimation_carry_over", "--acclimation_prior", "4"], monkeypatch, passes=2)
    s0, s1, s2 = seen["states"]
    assert _counters(s0) == [4] and _counters(s1) == [6] and _counters(s2) == [8]              # prior + 2 x images
    assert any(not torch.equal(s1[k], s2[k]) for k in s1 if k.endswith("running_mean"))
    assert all(int(b.old_num_batches_tracked) == 4 for _, b in _bns(seen["model"], BatchNorm2d))


def test_momentum_flag_reaches_every_layer(monkeypatch):
    seen = _passes(_ARGV + ["--acclimate_norm", "--acclimation_momentum", "0.25", "--early_stop", "0"], monkeypatch, passes=1)
    assert all(b.momentum == 0.25 for _, b in _bns(seen["model"], BatchNorm2d))
    assert _counters(seen["states"][1]) == [17]


def test_a_pass_without_the_flag_leaves_the_state_dict_alone(monkeypatch):
    seen = _passes(_ARGV, monkeypatch, passes=1)
    assert not _bns(seen["model"], BatchNorm2d)
    before, after = seen["states"]
    assert sorted(before) == sorted(after)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert not hasattr(seen["model"], "acclimate_norm")


# ---- kernel resources ----------------------------------------------------------------------------------------------------------------

def test_no_kernel_of_the_statistics_file_uses_scratch():
    from tests._kernel_resources import kernel_resources
    out = kernel_resources("dib_bnstats.hip")
    for frag, count in (("bn_partial_kernel", 1), ("bn_finalize_kernel", 1), ("bn_acclimate_finalize_kernel", 1), ("bn_apply_kernel", 4),
                        ("bn_apply_bump_kernel", 4)):
        assert len([n for n in out if frag in n]) == count, (frag, sorted(out))
    assert len(out) == 11, sorted(out)
    for n, r in out.items():
        assert r["ScratchSize"] == 0, (n, r)
        assert r["Occupancy"] >= 4, (n, r)


if __name__ == "__main__":
    if "--write" in sys.argv:
        np.savez_compressed(GOLDEN, **build_fixture())
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
