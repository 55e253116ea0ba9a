"""`--blur_acc_mode` on the GPU: what the engines launch in each of the four arithmetics, against the oracle's restatement of that
arithmetic bit for bit and against the bit-exact result within the mode's stated tolerance.

  (a) a ragged batch staged by engine._to_device and blurred by blur_image_list, with the engine's tables and without (blur_step);
  (b) a batch for which the large LDS window pays: fp32 / fast16 stay on the standard window, bitexact / fma16 give the same bits
      on either window;
  (c) PSFs on the 256 canvas: fast16 runs fma16's row-major loop, fp32 is served as it is;
  (d) the fused blur + normalise + pad launch in fp32 and fast16 against the two launches it replaces;
  (e) three training steps of the toy detector in fast16, fused epilogue on and off;
  (f) the three drivers' `main()` with the flag, each in a process of its own;
  (g) the grown boxes, identical in every mode.

Tolerances (absolute, images in [0, 1]) are the project's stated ones: fp32 5e-3 (tests/test_oracle_golden.py:88), fma16 1e-2
(tests/test_oracle_golden.py:103), fast16 1e-2 (tests/test_fast16_gpu.py:15)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import dib_oracle as O

pytestmark = pytest.mark.gpu

TOL = {"bitexact": 0.0, "fp32": 5e-3, "fma16": 1e-2, "fast16": 1e-2}
MODES = list(TOL)


def _const(mode):
    from detectinblur_amd import blur_ops
    return blur_ops.ACC_MODES[mode]


def _restated(mode, img, psf_norm, K=128):
    """The oracle's restatement of what `mode` computes for one image (the issue's table; fast16 at K = 256 is fma16's)."""
    if mode == "bitexact":
        return O.manual_blur(img, psf_norm)
    if mode == "fp32":
        return O.manual_blur(img, psf_norm, fp32_accumulate=True)
    if mode == "fma16" or K != 128:
        return O.manual_blur(img, psf_norm, fma16=True)
    rows, cols, _ = O.taps_of(psf_norm)
    return O.manual_blur(img, psf_norm, fma16=True, tap_order=O.tap_order_vruns(rows, cols))


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint16)


def _band_psf(rs, length, thick):
    """A thick, slanted band like a rasterised trajectory (several segments; every tap has vertical neighbours)."""
    a = np.zeros((128, 128), np.float64)
    x, y = 63.0 - length / 3, 63.0 - length / 2
    for _ in range(length * 3):
        x += rs.uniform(0.0, 0.5); y += rs.uniform(0.1, 0.45)
        for dy in range(thick):
            for dx in range(2):
                a[int(np.clip(y + dy, 0, 127)), int(np.clip(x + dx, 0, 127))] += rs.random_sample() + 0.1
    return a / a.sum()


def _dict(psf, **extra):
    d = {"blurring": True, "psf": psf, "theta_rad": 0.25, "scale_factor_lambda1": 0.9, "scale_factor_lambda2": 0.8,
         "param_index": 0, "fraction_index": 0}
    d.update(extra)
    return d


_SHARP = {"blurring": False, "psf": [0], "theta_rad": 0, "scale_factor_lambda1": 1, "scale_factor_lambda2": 1, "param_index": None,
          "fraction_index": None}


class Batch(object):
    """A batch as the loader hands it over (fp32 CPU images holding fp16 values, targets, blur_dicts) with, per mode, the oracle's
    result for every image -- computed once and shared by the tests that need it."""

    def __init__(self, shapes, psfs, seed, extra=None):
        rs = np.random.RandomState(seed)
        self.half = [rs.random_sample(s).astype(np.float16) for s in shapes]
        self.images = [torch.from_numpy(h.astype(np.float32)) for h in self.half]
        self.dicts = [dict(_SHARP) if p is None else _dict(p, **(extra[i] if extra else {})) for i, p in enumerate(psfs)]
        self.norm = [None if p is None else O.normalize_psf(O.to_half_like_torch(p)) for p in psfs]      # what the compaction makes of it
        self.K = next(p.shape[0] for p in psfs if p is not None)
        self.targets = []
        for i, s in enumerate(shapes):
            x1, y1 = rs.uniform(0, s[2] - 12, 3), rs.uniform(0, s[1] - 12, 3)
            b = np.stack([x1, y1, np.minimum(x1 + rs.uniform(4, s[2] / 2, 3), s[2]), np.minimum(y1 + rs.uniform(4, s[1] / 2, 3), s[1])], 1)
            self.targets.append({"boxes": torch.from_numpy(b.astype(np.float32)), "labels": torch.tensor([1, 2, 3]), "image_id": torch.tensor([i])})
        self._want = {}

    def want(self, mode):
        if mode not in self._want:
            self._want[mode] = [h if n is None else _restated(mode, h, n, self.K) for h, n in zip(self.half, self.norm)]
        return self._want[mode]

    def stage(self, mode):
        from detectinblur_amd import engine
        return engine._to_device(self.images, [dict(t) for t in self.targets], self.dicts, torch.device("cuda"), True, want_tables=True,
                                 blur_acc_mode=mode)


@functools.lru_cache(maxsize=None)
def _ragged():
    import bench
    gen = bench.make_psfs_host(0)[0]                     # generated low-exposure PSFs (fractions 1/18 .. 1/5)
    one = np.zeros((128, 128), np.float64); one[63, 63] = 1.0
    rs = np.random.RandomState(77)
    return Batch([(3, 97, 150), (3, 67, 129), (3, 80, 100), (3, 70, 200), (3, 97, 150)],
                 [gen[0], gen[1], None, _band_psf(rs, 40, 5), one], seed=5)


def _check(batch, mode, images, exact=None):
    want = batch.want(mode)
    for i, (g, w) in enumerate(zip(images, want)):
        assert g.dtype == torch.float16 and tuple(g.shape) == w.shape, (mode, i)
        assert np.array_equal(_bits(g), w.view(np.uint16)), (mode, i)
    if exact is not None:
        worst = max(float((g.float() - e.float()).abs().max()) for g, e in zip(images, exact))
        print("%s: max |mode - bitexact| = %.3e (stated %.0e)" % (mode, worst, TOL[mode]))
        assert worst <= TOL[mode], (mode, worst)


def _blur(batch, mode, with_tables):
    from detectinblur_amd.models import blur_functions as BF
    images, _t, psfs, _th, _l1, _l2, tables = batch.stage(mode)
    assert tables is not None
    BF.blur_image_list(images, batch.dicts, psfs_GPU=psfs, acc_mode=_const(mode), tables=tables if with_tables else None)
    return images, tables


# ---- (a) ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_tables", [True, False], ids=["tables", "blur_step"])
@pytest.mark.parametrize("mode", MODES)
def test_engine_path_equals_the_restated_arithmetic(mode, with_tables):
    batch = _ragged()
    images, tables = _blur(batch, mode, with_tables)
    assert tables.vruns is (mode == "fast16") and not tables.large
    exact, _ = _blur(batch, "bitexact", with_tables)
    _check(batch, mode, images, exact)
    assert np.array_equal(_bits(images[2]), batch.half[2].view(np.uint16))      # the image that is not blurred


# ---- (b) ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _refill_heavy():
    """Two images under 10 x 40 block PSFs: 40 columns are two standard segments per row (20) and ONE large one."""
    from detectinblur_amd import blur_ops, transforms as T
    rs = np.random.RandomState(3)
    psfs, extra = [], []
    for _ in range(2):
        a = np.zeros((128, 128), np.float64)
        a[58:68, 44:84] = rs.random_sample((10, 40)) + 0.05
        psfs.append(a / a.sum())
        extra.append({"psf_taps": 400, "psf_segments": (T.count_tap_segments(a, T.STANDARD_WINDOW), T.count_tap_segments(a, T.LARGE_WINDOW))})
    b = Batch([(3, 70, 130), (3, 65, 97)], psfs, seed=11, extra=extra)
    assert blur_ops.large_window_pays(b.dicts, 2)
    return b


@pytest.mark.parametrize("with_tables", [True, False], ids=["tables", "blur_step"])
@pytest.mark.parametrize("mode", MODES)
def test_large_window_regime(mode, with_tables):
    from detectinblur_amd import blur_ops
    from detectinblur_amd.models import blur_functions as BF
    batch = _refill_heavy()
    images, tables = _blur(batch, mode, with_tables)
    assert tables.large is (mode in ("bitexact", "fma16")) and tables.vruns is (mode == "fast16")
    _check(batch, mode, images)                              # fp32 and fast16 (standard window) still equal their restatements
    if mode in ("bitexact", "fma16"):                        # ... and these two their own standard-window result
        staged = batch.stage(mode)
        std_tables = blur_ops.compact_psfs([p for p in staged[2]], normalize=True)
        std = list(staged[0])
        BF.blur_image_list(std, batch.dicts, psfs_GPU=staged[2], acc_mode=_const(mode), tables=std_tables)
        assert not std_tables.large
        for a, b in zip(images, std):
            assert torch.equal(a, b)


# ---- (c) ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _canvas256():
    rs = np.random.RandomState(21)
    psfs = []
    for n, spread in ((25, 30), (60, 12)):
        a = np.zeros((256, 256), np.float64)
        a[np.clip(rs.randint(-spread, spread + 1, n) + 127, 0, 255), np.clip(rs.randint(-spread, spread + 1, n) + 127, 0, 255)] = rs.random_sample(n) + 0.05
        psfs.append(a / a.sum())
    return Batch([(3, 70, 90), (3, 97, 150)], psfs, seed=13)


@pytest.mark.parametrize("with_tables", [True, False], ids=["tables", "blur_step"])
@pytest.mark.parametrize("mode", MODES)
def test_canvas_256(mode, with_tables):
    """--dont_center_psf: fast16 equals the fma16 restatement (row-major order), fp32 its own."""
    batch = _canvas256()
    images, tables = _blur(batch, mode, with_tables)
    assert tables.K == 256 and not tables.vruns
    exact, _ = _blur(batch, "bitexact", with_tables)
    _check(batch, mode, images, exact)
    if mode == "fast16":
        for g, w in zip(images, batch.want("fma16")):
            assert np.array_equal(_bits(g), w.view(np.uint16))


# ---- (d) ------------------------------------------------------------------------------------------------------------

def _psf(rs, n, spread, K=128):
    a = np.zeros((K, K), np.float64)
    c = K // 2 - 1
    a[np.clip(rs.randint(-spread, spread + 1, n) + c, 0, K - 1), np.clip(rs.randint(-spread, spread + 1, n) + c, 0, K - 1)] = rs.random_sample(n) + 0.05
    return torch.from_numpy(O.to_half_like_torch(a)).cuda()


@pytest.mark.parametrize("channels_last", [False, True], ids=["planar", "channels_last"])
@pytest.mark.parametrize("shape", [(3, 96, 250, 96, 256), (5, 70, 130, 96, 256), (2, 65, 128, 96, 128)])
@pytest.mark.parametrize("mode", ["fp32", "fast16"])
def test_fused_launch_equals_blur_then_normalize_pad(mode, shape, channels_last):
    from detectinblur_amd import blur_ops
    B, H, W, Hp, Wp = shape
    rs = np.random.RandomState(B * 1000 + H)
    images = [torch.from_numpy(rs.random_sample((3, H, W)).astype(np.float16)).cuda() for _ in range(B)]
    # scattered taps AND dense blocks (vertical runs of every length for fast16)
    psfs = [_psf(rs, 5 + 9 * i, 2 + 3 * i) for i in range(B)]
    psfs[0][60:67, 62:65] = 0.07
    acc, vruns, _ = blur_ops.resolve_acc_mode(mode, 128, torch.float16)
    tables = blur_ops.compact_psfs(psfs, normalize=True, vruns=vruns)
    means, stds = rs.uniform(0.2, 0.6, (B, 3)), rs.uniform(0.15, 0.35, (B, 3))
    index = list(range(B))
    want = blur_ops.normalize_pad(blur_ops.sparse_blur(list(images), index, tables, acc), means, stds, Hp, Wp, channels_last)
    got = blur_ops.sparse_blur_normalized(images, index, tables, means, stds, Hp, Wp, channels_last, acc, order=sorted(index, reverse=True))
    assert got is not None and got.shape == want.shape and got.stride() == want.stride()
    assert torch.equal(got, want)                  # every pixel AND every padding zero
    exact = blur_ops.normalize_pad(blur_ops.sparse_blur(list(images), index, tables), means, stds, Hp, Wp, channels_last)
    assert not torch.equal(got, exact)             # (the mode's own arithmetic ran, not the default's)


def test_fused_launch_does_not_serve_fast16_on_the_256_canvas_or_without_groups():
    from detectinblur_amd import _lib, blur_ops
    rs = np.random.RandomState(4)
    images = [torch.from_numpy(rs.random_sample((3, 96, 128)).astype(np.float16)).cuda() for _ in range(2)]
    means, stds = rs.uniform(0.2, 0.6, (2, 3)), rs.uniform(0.15, 0.35, (2, 3))
    t256 = blur_ops.compact_psfs([_psf(rs, 12, 5, 256) for _ in range(2)], normalize=True)
    assert blur_ops.sparse_blur_normalized(images, [0, 1], t256, means, stds, 96, 128, False, _lib.DIB_ACC_FAST16) is None
    # ... and fp32 at K = 256 is served
    want = blur_ops.normalize_pad(blur_ops.sparse_blur(list(images), [0, 1], t256, _lib.DIB_ACC_FP32), means, stds, 96, 128)
    got = blur_ops.sparse_blur_normalized(images, [0, 1], t256, means, stds, 96, 128, False, _lib.DIB_ACC_FP32)
    assert got is not None and torch.equal(got, want)
    plain = blur_ops.compact_psfs([_psf(rs, 12, 5) for _ in range(2)], normalize=True)
    with pytest.raises(ValueError, match="vruns=True"):
        blur_ops.sparse_blur_normalized(images, [0, 1], plain, means, stds, 96, 128, False, _lib.DIB_ACC_FAST16)


# ---- (e) ------------------------------------------------------------------------------------------------------------

def test_three_training_steps_in_fast16(monkeypatch):
    """The toy detector of tests/test_blur_normalized_gpu.py's training-loop test, three steps: in fast16 the weights are the same
    bit for bit with FUSE_BLUR_EPILOGUE on and off (the fused launch serves the mode), they are NOT the bit-exact run's, and the
    first blurred batch lies within 1e-2 of the bit-exact one."""
    import contextlib
    import io
    import pin_inputs as PI
    from detectinblur_amd import engine
    from detectinblur_amd.models import blur_functions as BF
    from detectinblur_amd.models.net_transforms import GeneralizedRCNNTransform

    class Wrapped(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.core = PI.ToyDetector(3)
            self.transform = GeneralizedRCNNTransform(96, 160, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
            self.transform.channels_last = True

        def forward(self, images, targets=None, thetas=None, lambda1s=None, lambda2s=None, newMeans=None, newSTDs=None):
            batch, targets = self.transform(images, targets, newMeans, newSTDs)
            imgs = [batch.tensors[i] * 0.25 + 0.5 for i in range(batch.tensors.shape[0])]
            n = len(imgs)
            return self.core(imgs, targets, newMeans=np.zeros((n, 3)), newSTDs=np.ones((n, 3)))

    def loader():
        rs = np.random.RandomState(99)
        out = PI.ListLoader()
        for k in range(3):
            images = tuple(torch.from_numpy(rs.random_sample((3, 96, 160)).astype(np.float32)) for _ in range(2))
            targets = tuple(PI._target(rs, 96, 160, 3, 10 * k + j) for j in range(2))
            dicts = tuple(dict(PI._blur_dict(rs, (k + j) % 3, (2 * k + j) % 5, True), psf_taps=5 + j) for j in range(2))
            out.append((images, targets, dicts))
        return out

    def run(flag, mode):
        monkeypatch.setattr(engine, "FUSE_BLUR_EPILOGUE", flag)
        torch.manual_seed(0)
        np.random.seed(0)
        model = Wrapped().cuda()
        opt = torch.optim.SGD(model.parameters(), lr=0.04, momentum=0.9)
        with contextlib.redirect_stdout(io.StringIO()):
            engine.train_one_epoch(model, opt, loader(), torch.device("cuda"), epoch=1, print_freq=10, writer=PI.RecordingWriter(),
                                   blur_train=True, gpu_blur=True, expand_target_boxes=True, use_custom_image_norm=True, blur_acc_mode=mode)
        return {k: v.detach().clone() for k, v in model.state_dict().items()}, getattr(model.transform, "last_epilogue", None)

    plain, how_plain = run(False, "fast16")
    fused, how_fused = run(True, "fast16")
    exact, _ = run(False, "bitexact")
    assert how_plain is None and how_fused == "fused into the blur"
    for k in plain:
        assert torch.equal(plain[k], fused[k]), k
    assert any(not torch.equal(plain[k], exact[k]) for k in plain)

    images_CPU, targets, dicts = loader()[0]
    got = {}
    for mode in ("bitexact", "fast16"):
        images, _t, psfs, _th, _l1, _l2, tables = engine._to_device(images_CPU, targets, dicts, torch.device("cuda"), True, blur_acc_mode=mode)
        BF.blur_image_list(images, dicts, psfs_GPU=psfs, acc_mode=_const(mode), tables=tables)
        got[mode] = images
    worst = max(float((a.float() - b.float()).abs().max()) for a, b in zip(got["fast16"], got["bitexact"]))
    print("first blurred batch: max |fast16 - bitexact| = %.3e" % worst)
    assert 0.0 < worst <= TOL["fast16"]


# ---- (f) ------------------------------------------------------------------------------------------------------------

def _run_child(target, tmp_path, *args, timeout=900):
    from detectinblur_amd import utils
    ctx = utils.loader_context()
    if ctx is None:
        pytest.skip("no fork server (the GPU was initialised before the test session could start one)")
    out = str(tmp_path / "child.json")
    p = ctx.Process(target=target, args=(out,) + args)
    p.start()
    p.join(timeout)
    if p.is_alive():
        p.kill()
        p.join()
        pytest.fail("child timed out")
    if os.path.exists(out + ".err"):
        pytest.fail(open(out + ".err").read()[-4000:])
    assert p.exitcode == 0 and os.path.exists(out), p.exitcode
    return json.load(open(out))


_SIZES = ["--synthetic", "--synthetic_images", "4", "--synthetic_size", "96", "160"]
_DRIVERS = {
    "train": _SIZES + ["--min_size", "96", "--max_size", "160", "--blur_train", "--gpu_blur", "-b", "2", "--epochs", "1", "--early_stop", "0",
                       "--lr", "0.001", "--print_freq", "1", "--output_dir", "", "--tensorboard_path", ""],
    "evaluate": _SIZES + ["--min_size", "96", "--max_size", "160", "--blur_eval", "--gpu_blur", "--early_stop", "1", "--tensorboard_path", ""],
    # (the estimator's parser has no --min_size / --max_size: its batcher is fixed at 800 x 1333)
    "train_blur_estimator": _SIZES + ["--blur_train", "--gpu_blur", "--LEHE_blur_seg", "-b", "2", "--epochs", "1", "--early_stop", "0",
                                      "--lr", "0.001", "--print_freq", "1", "--output_dir", ""],
}


@pytest.mark.parametrize("which", list(_DRIVERS))
def test_driver_main_runs_in_fast16(tmp_path, which):
    """Every launch of the blur that the driver makes is asked for DIB_ACC_FAST16, on tables that carry the vertical-run groups
    where the caller owns the tables (sparse_blur; blur_step's are the library's, which compacts them with the groups itself);
    losses, COCO statistics and accuracies come out finite."""
    from detectinblur_amd import _lib
    from tests import _blur_acc_mode_children as C
    r = _run_child(C.driver, tmp_path, which, _DRIVERS[which] + ["--blur_acc_mode", "fast16"])
    print(json.dumps({k: v for k, v in r.items() if k != "tail"}))
    assert r["calls"], r["tail"]
    for c in r["calls"]:
        assert c["acc_mode"] == _lib.DIB_ACC_FAST16 and c["K"] == 128, c
        if c["entry"] == "sparse_blur":
            assert c["vruns"] and not c["large"], c
    assert r["finite"], r
    if which == "train_blur_estimator":
        assert r["losses"] and r["accuracies"]
    else:
        assert r["stats"] and all(len(s) == 12 for s in r["stats"])
        assert any(c["entry"] == "sparse_blur" for c in r["calls"])
    if which == "train":
        assert r["losses"]


# ---- (g) ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("make", [_ragged, _refill_heavy], ids=["ragged", "large_window_regime"])
def test_boxes_are_the_same_in_every_mode(make):
    """utils.expand_targets(tables=) reads the tap list, not the segments or the groups."""
    from detectinblur_amd import utils
    batch = make()
    want = [t["boxes"].numpy() if n is None else O.expand_boxes(t["boxes"].numpy(), n, h.shape[1], h.shape[2])
            for t, n, h in zip(batch.targets, batch.norm, batch.half)]
    for mode in MODES:
        images, targets, psfs, _th, _l1, _l2, tables = batch.stage(mode)
        out = utils.expand_targets(targets, batch.dicts, psfs, images, tables=tables)
        for i, (t, w) in enumerate(zip(out, want)):
            assert np.array_equal(t["boxes"].cpu().numpy(), w), (mode, i)
