"""The estimator's input batch in one launch (csrc/dib_epilogue.hip: dib_normalize_resize_crop -- optional 8-bit quantisation, float
conversion, normalisation, bilinear resize, top-left crop) against the module-by-module path of
GeneralizedRCNNTransform(crop_images=True) with `fused = False`, which stays the checker: bit for bit, through the kernel's own
wrapper, the transform, both estimator loops, the ensemble's router input and the driver."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import pin_inputs as PI
from detectinblur_amd import blur_ops
from detectinblur_amd import engine_blur_estimator as EB
from detectinblur_amd.models.net_transforms import GeneralizedRCNNTransform

pytestmark = pytest.mark.gpu
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def _images(dtype, sizes, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(3, h, w, generator=g).to(dtype).cuda() for h, w in sizes]


def _both(imgs, min_size, max_size, channels_last=False, training=True, targets=True, quantize=False):
    """(tensors, image_sizes, boxes, next generator value) of the crop batcher, fused and module by module."""
    out = {}
    for fused in (True, False):
        t = GeneralizedRCNNTransform(min_size, max_size, MEAN, STD, crop_images=True, training=training)
        t.fused, t.channels_last = fused, channels_last
        tg = [{"boxes": torch.tensor([[1.0, 2.0, 30.0, 40.0], [5.5, 6.25, 20.0, 33.0]]).cuda()} for _ in imgs] if targets else None
        torch.manual_seed(3)
        if quantize:
            t.pending_quantize = True
        il, res = t([i.clone() for i in imgs], tg)
        assert "pending_quantize" not in t.__dict__                     # one call
        out[fused] = (il.tensors, il.image_sizes, [d["boxes"] for d in res] if targets else [], torch.rand(1).item())
    return out[True], out[False]


def _assert_equal(a, b, channels_last=False):
    assert a[0].dtype == torch.float32 and a[0].shape == b[0].shape
    assert a[0].is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    assert a[1] == b[1] and a[3] == b[3]                                # resized sizes, generator state
    assert torch.equal(a[0], b[0])
    assert len(a[2]) == len(b[2]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


CASES = {
    # down, up, identity (its size a multiple of 32): crop 64 x 64
    "down_up_identity": (64, 128, [(70, 100), (48, 60), (64, 96)], (64, 64)),
    # a crop wider than one 256-column block
    "two_x_blocks": (96, 400, [(96, 300), (100, 330), (97, 317)], (96, 288)),
    # image 1 resizes to exactly the crop (64 x 96): its last source row and column are read (h1p = w1p = 0)
    "resized_equals_crop": (64, 128, [(128, 200), (32, 48), (80, 121)], (64, 96)),
    "batch_of_one": (64, 128, [(50, 77)], (64, 96)),
}


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_fused_crop_equals_the_module_path_bit_for_bit(case, channels_last, dtype):
    min_size, max_size, sizes, crop = CASES[case]
    a, b = _both(_images(dtype, sizes, seed=4), min_size, max_size, channels_last)
    assert tuple(a[0].shape) == (len(sizes), 3) + crop, a[0].shape
    if case == "resized_equals_crop":
        assert a[1][1] == crop
    if case == "down_up_identity":
        assert a[1][2] == (64, 96)
    _assert_equal(a, b, channels_last)


def test_fused_crop_of_33_images_crosses_the_chunk_of_32():
    a, b = _both(_images(torch.float16, [(33, 40)] * 33, seed=5), 64, 128, channels_last=True)
    assert tuple(a[0].shape) == (33, 3, 64, 64)
    _assert_equal(a, b, True)
    assert not torch.equal(a[0][32], a[0][0])                           # image 32 is its own, not a re-read of chunk 0


def test_a_crop_of_no_pixels_goes_through_the_module_path(monkeypatch):
    calls = []
    monkeypatch.setattr(blur_ops, "normalize_crop", lambda *a, **k: calls.append(1))
    a, b = _both(_images(torch.float16, [(20, 300), (64, 96)], seed=6), 64, 128)      # 20 x 300 -> 8 x 128: floor(8 / 32) = 0
    assert not calls and a[0].shape[2] == 0
    _assert_equal(a, b)


def test_the_entry_point_refuses_a_crop_an_image_does_not_cover():
    imgs = _images(torch.float16, [(40, 70), (64, 33)])
    blur_ops.normalize_crop(imgs, [MEAN] * 2, [STD] * 2, 32, 32)
    with pytest.raises(Exception, match="smaller than the crop"):
        blur_ops.normalize_crop(imgs, [MEAN] * 2, [STD] * 2, 32, 64)
    with pytest.raises(Exception, match="fp16"):
        blur_ops.normalize_crop([i.float() for i in imgs], [MEAN] * 2, [STD] * 2, 32, 32, quantize=True)
    with pytest.raises(Exception, match="larger than the batch"):
        blur_ops.normalize_pad(imgs, [MEAN] * 2, [STD] * 2, 32, 96, quantize=True)


# ---- the quantisation, over every Half ---------------------------------------------------------------------------------------

def test_quantise_flag_equals_the_torch_expression_for_every_half_in_the_domain():
    """All 65,536 bit patterns as one 3 x 128 x 512 image (every pattern once per plane, the three planes in three orders).  Domain
    (include/dib.h): finite x >= 0 with half(x * 255) < 256.  There the flagged launch equals the reference's expression followed by
    the unflagged launch, bit for bit, in crop and pad mode, with and without a resize behind it.  Outside the domain the figures
    are printed, not asserted (DESIGN.md section 4 says what they are)."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    planes = torch.stack([bits, bits.flip(0), bits.roll(12345)]).view(3, 128, 512)
    x = planes.view(torch.float16).cuda()
    scaled = x * 255
    domain = torch.isfinite(x) & (x >= 0) & (scaled < 256)
    assert int(domain[0].sum()) == 15364 + 1                            # +0 .. 0x3C03 (1.0029297), and -0
    q = GeneralizedRCNNTransform.quantize(x)
    assert q.dtype == torch.float16
    want = blur_ops.normalize_crop([q], [MEAN], [STD], 128, 512)
    got = blur_ops.normalize_crop([x], [MEAN], [STD], 128, 512, quantize=True)
    same = (got.view(torch.int32) == want.view(torch.int32))[0]
    outside = ~domain
    print("quantise, outside the domain: %d patterns per plane, %d equal to ATen's result bit for bit; differing: %s"
          % (int(outside[0].sum()), int((same & outside)[0].sum()),
             sorted({"%04x" % (int(b) & 0xFFFF) for b in planes.cuda()[0][(~same & outside)[0]][:16].tolist()})))
    assert bool(same[domain].all())
    pad = blur_ops.normalize_pad([x], [MEAN], [STD], 128, 512, quantize=True)
    assert bool((pad.view(torch.int32) == want.view(torch.int32))[0][domain].all())
    # with the resize behind it: an image of domain values only (every k / 255 and its neighbours), through the transform
    g = torch.Generator().manual_seed(8)
    img = (torch.rand(3, 70, 100, generator=g) * 1.002).half().cuda()
    assert bool((img * 255 < 256).all())
    a, b = _both([img, img.flip(-1)[:, :48, :60].contiguous()], 64, 128, channels_last=True, quantize=True)
    _assert_equal(a, b, True)
    # ... and the module path given `pending_quantize` quantises, too (it is not the identity on this image)
    plain, _ = _both([img, img.flip(-1)[:, :48, :60].contiguous()], 64, 128, channels_last=True, quantize=False)
    assert plain[0].shape == a[0].shape and not torch.equal(plain[0], a[0])


# ---- deferred AugMix through the estimator's staging ---------------------------------------------------------------------------

def test_deferred_augmix_plans_through_the_estimators_staging():
    from detectinblur_amd import augmix
    rs = np.random.RandomState(2)
    images = [torch.from_numpy(rs.randint(0, 256, (3, 48, 64)).astype(np.float32) / np.float32(255)) for _ in range(4)]
    np.random.seed(11)
    plans = [augmix.draw_plan(48, 64, positional=False)[0]]
    while len(plans) < 3:                                               # two plans with positional ops, the second one mirrored
        plan = augmix.draw_plan(48, 64, positional=True)[0]
        if any(op in augmix.POSITIONAL_OPS for chain in plan["chains"] for op, _ in chain):
            plans.append(plan)
    for plan in plans:
        plan["deferred"] = True
    plans[2]["flip"] = True
    plans.append(None)
    dicts = [{"blurring": False, "psf": [0], "param_index": None, "fraction_index": None} for _ in images]
    for bd, plan in zip(dicts, plans):
        if plan is not None:
            bd["augmix"] = plan
    targets = [{"boxes": torch.tensor([[1.0, 2.0, 30.0, 40.0]])} for _ in images]
    staged, tg, psfs, tables = EB._stage(images, targets, dicts, torch.device("cuda"), False)
    assert psfs is None and tables is None and all(t["boxes"].is_cuda for t in tg)
    for got, image, plan in zip(staged, images, plans):
        want = (image if plan is None else augmix.apply_deferred_host(image, plan)).half()
        assert got.dtype == torch.float16 and torch.equal(got.cpu(), want)
    assert not torch.equal(staged[0].cpu(), images[0].half())           # the plan did something


# ---- the loops --------------------------------------------------------------------------------------------------------------------

def _unfuse(monkeypatch, only_crop=False):
    """Every batcher built from here on takes the module path."""
    init = GeneralizedRCNNTransform.__init__

    def unfused(self, *a, **k):
        init(self, *a, **k)
        if self.crop_images or not only_crop:
            self.fused = False
    monkeypatch.setattr(GeneralizedRCNNTransform, "__init__", unfused)


def _loader(train):
    rs = np.random.RandomState(40 + train)
    loader = PI.ListLoader()
    for k in range(2):
        n = 4 if train else 1
        images = tuple(torch.from_numpy(rs.random_sample((3, 96, 128)).astype(np.float32)) for _ in range(n))
        targets = tuple(PI._target(rs, 96, 128, 2, 10 * k + j) for j in range(n))
        dicts = tuple(PI._blur_dict(rs, (k + j) % 3, (2 * k + j) % 5, j != 1) for j in range(n))
        loader.append((images, targets, dicts))
    loader.dataset = object()
    return loader


def _run_loops():
    torch.manual_seed(0)
    np.random.seed(0)
    model = PI.ToyClassifier(16, 1).cuda()
    opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9)
    criterion, losses = torch.nn.CrossEntropyLoss(), []

    def crit(output, target):
        loss = criterion(output, target)
        losses.append(float(loss.detach()))
        return loss
    kw = dict(quantize_image=True, gpu_blur=True)
    with contextlib.redirect_stdout(io.StringIO()):
        EB.train_one_epoch(model, opt, crit, _loader(True), torch.device("cuda"), print_freq=1, crop_images=True, blur_train=True, **kw)
        logits = []
        hook = model.register_forward_hook(lambda m, i, o: logits.append(o.detach().clone()))
        acc = EB.evaluate(model, _loader(False), torch.device("cuda"), blurring_images=True, **kw)
        hook.remove()
    return losses, [m["shape"] for m in model.calls], {k: v.clone() for k, v in model.state_dict().items()}, logits, acc


def test_estimator_loops_are_identical_with_and_without_the_fused_batcher(monkeypatch):
    """train_one_epoch (crop batcher, quantise handed to the crop launch) and evaluate (pad batcher, quantise handed to the pad
    launch) on blurred 96 x 128 images, b = 4: losses, weights, logits and accuracies equal the module path's bit for bit."""
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True          # the toy convolution's backward must be the same run to run
    launches = []
    crop, pad = blur_ops.normalize_crop, blur_ops.normalize_pad
    try:
        with monkeypatch.context() as mp:
            mp.setattr(blur_ops, "normalize_crop", lambda *a, **k: launches.append(("crop", k.get("quantize"), a[0][0].dtype)) or crop(*a, **k))
            mp.setattr(blur_ops, "normalize_pad", lambda *a, **k: launches.append(("pad", k.get("quantize"), a[0][0].dtype)) or pad(*a, **k))
            fused = _run_loops()
            assert launches == [("crop", True, torch.float16)] * 2 + [("pad", True, torch.float16)] * 2
            _unfuse(mp)
            unfused = _run_loops()
            assert len(launches) == 4
    finally:
        torch.backends.cudnn.deterministic = det
    assert fused[1] == unfused[1] and fused[1][0] == [4, 3, 800, 1056] and fused[1][-1] == [1, 3, 800, 1088]
    assert len(fused[0]) == 2 and fused[0] == unfused[0]
    assert all(torch.equal(fused[2][k], unfused[2][k]) for k in fused[2])
    assert len(fused[3]) == 2 and all(torch.equal(x, y) for x, y in zip(fused[3], unfused[3]))
    assert fused[4] == unfused[4]


def test_the_ensembles_estimator_input_is_identical_fused_and_module_by_module(monkeypatch):
    """engine.evaluate builds the same crop batcher for the ensemble's router (engine.py: `batcher(images_GPU, None)` -> _estimate):
    one 160 x 224 image, the tensor `_estimate` receives."""
    from detectinblur_amd import engine, utils
    from detectinblur_amd.coco_utils import SyntheticCocoDetection
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    from detectinblur_amd.train import get_transform
    import random
    torch.manual_seed(0)
    det = fasterrcnn_resnet50_fpn(pretrained=False, pretrained_backbone=False, num_classes=91, min_size=160, max_size=224,
                                  rpn_post_nms_top_n_test=50).cuda()
    est = PI.ToyClassifier(4, 2).cuda()
    random.seed(3); np.random.seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        ds = SyntheticCocoDetection(num_images=1, size=(160, 224), boxes_per_image=3,
                                    transforms=get_transform(False, blur=True, blur_type=0.005, blur_ratio=1.0, low_exposure=True))
    batch = utils.collate_fn([ds[0]])

    class L(list):
        dataset = ds
    seen = []
    plain = engine._estimate
    monkeypatch.setattr(engine, "_estimate", lambda m, x, graphed: seen.append(x.clone()) or plain(m, x, graphed))
    launches = []
    crop = blur_ops.normalize_crop
    monkeypatch.setattr(blur_ops, "normalize_crop", lambda *a, **k: launches.append(1) or crop(*a, **k))
    kw = dict(blurring_images=True, gpu_blur=True, use_ensemble=True, ensemble_models=[det] * 4, blur_estimator=est, LEHE=True)
    with contextlib.redirect_stdout(io.StringIO()):
        engine.evaluate(None, L([batch]), torch.device("cuda"), **kw)
        assert len(launches) == 1
        _unfuse(monkeypatch, only_crop=True)
        engine.evaluate(None, L([batch]), torch.device("cuda"), **kw)
    assert len(launches) == 1 and len(seen) == 2
    assert tuple(seen[0].shape) == (1, 3, 800, 1120) and torch.equal(seen[0], seen[1])


def test_driver_trains_with_augmix_the_fused_input_and_tensorboard(tmp_path, monkeypatch):
    from detectinblur_amd import tb_writer
    from detectinblur_amd import train_blur_estimator as TB
    monkeypatch.chdir(tmp_path)
    launches = []
    crop = blur_ops.normalize_crop
    monkeypatch.setattr(blur_ops, "normalize_crop", lambda *a, **k: launches.append(k.get("quantize")) or crop(*a, **k))
    args = TB.build_parser().parse_args([
        "--synthetic", "--synthetic_images", "8", "--synthetic_size", "96", "128", "--blur_train", "--gpu_blur", "--crop_images",
        "--quantize_image", "--non_pos_aug_mix", "--include_pos_aug_mix", "-b", "4", "--epochs", "1", "--early_stop", "2",
        "--tensorboard_path", str(tmp_path / "tb"), "--output_dir", str(tmp_path / "est")])
    n_threads = torch.get_num_threads()
    try:
        with contextlib.redirect_stdout(io.StringIO()) as out:
            TB.main(args)
    finally:
        torch.set_num_threads(n_threads)
    assert "Top 1 Accuracy" in out.getvalue()
    assert launches == [True, True]                                     # 8 images, b = 4: both training batches, quantised in the launch
    assert (tmp_path / "est" / "blur_estimator_0.pth").exists()
    files = [f for f in os.listdir(str(tmp_path / "tb")) if f.startswith("events.out.tfevents.")]
    assert len(files) == 1
    tags = {tag for tag, _, _ in tb_writer.read_scalars(str(tmp_path / "tb" / files[0]))}
    assert {"losses/loss", "losses/overallLoss", "learningRate", "Blurred/Top1Accuracy", "Blurred/Top2Accuracy"} <= tags
