"""AugMix on the GPU (csrc/dib_augmix.hip via augmix.apply_plans_device) against the host path (augmix.apply_plan, the reference's
Pillow operations and float64 mix; tests/test_augmix.py pins that against the reference): the fp16 images equal `.half()` of the
host path's result bit for bit -- every op at its extreme parameters, flipped and unflipped, degenerate histograms, random plans,
b = 8 at 800 x 1333 and ragged sizes -- two runs are identical, and the training step's staging feeds the blur exactly those images."""
import copy
import random

import numpy as np
import pytest
import torch

from detectinblur_amd import augmix as A

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _host(img_u8, plan, flip):
    """float CHW k / 255 input (mirrored when flip) and the host path's fp16 result in the same frame."""
    x = torch.from_numpy(np.ascontiguousarray(img_u8.transpose(2, 0, 1))).to(torch.float32).div(255)
    if flip:
        x = x.flip(-1).contiguous()
    p = dict(plan, flip=flip, deferred=True)
    return x, A.apply_deferred_host(x, p).half(), p


def _check(imgs, plans, flips):
    xs, want, ps = zip(*[_host(i, p, f) for i, p, f in zip(imgs, plans, flips)])
    got = A.apply_plans_device([x.to(DEV) for x in xs], list(ps))
    torch.cuda.synchronize()
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.cpu()
        if not torch.equal(g.view(torch.int16), w.view(torch.int16)):
            bad = (g.float() - w.float()).abs()
            raise AssertionError("image %d (%s, flip %s): %d of %d values differ, max %g" % (k, ps[k]["chains"], flips[k],
                                                                                           int((bad > 0).sum()), bad.numel(), float(bad.max())))
    return got


def _plan(chains, ws=(0.2, 0.3, 0.5), m=0.7):
    ws = tuple(float(np.float32(w)) for w in ws)
    return {"ws": ws, "m": float(np.float32(m)), "chains": chains, "deferred": True, "flip": False}


def _image(rs, H, W, kind="random"):
    if kind == "constant":
        return np.full((H, W, 3), 77, np.uint8)
    if kind == "two":
        return np.where(rs.rand(H, W, 3) < 0.3, 12, 200).astype(np.uint8)
    if kind == "narrow":
        return rs.randint(100, 110, (H, W, 3)).astype(np.uint8)
    return rs.randint(0, 256, (H, W, 3)).astype(np.uint8)


def _extreme_chains(H, W):
    t = int(3.999 * (((W + H) / 2) / 3) / 10)
    ops = [[(A.AUTOCONTRAST, 0)], [(A.EQUALIZE, 0)], [(A.POSTERIZE, 1)], [(A.POSTERIZE, 4)], [(A.SOLARIZE, 1)], [(A.SOLARIZE, 256)],
           [(A.SOLARIZE, 128)], [(A.ROTATE, 11)], [(A.ROTATE, -11)], [(A.ROTATE, 0)], [(A.SHEAR_X, 0.1199)], [(A.SHEAR_X, -0.1199)],
           [(A.SHEAR_Y, 0.1199)], [(A.SHEAR_Y, -0.003)], [(A.TRANSLATE_X, t)], [(A.TRANSLATE_X, -t)], [(A.TRANSLATE_Y, t)],
           [(A.TRANSLATE_Y, -t)], [(A.TRANSLATE_X, 0)]]
    mixed = [[(A.EQUALIZE, 0), (A.ROTATE, 7), (A.AUTOCONTRAST, 0)], [(A.SHEAR_X, 0.05), (A.TRANSLATE_Y, -3), (A.ROTATE, -9)],
             [(A.POSTERIZE, 2), (A.SOLARIZE, 90), (A.EQUALIZE, 0)], [(A.ROTATE, 5), (A.EQUALIZE, 0), (A.SHEAR_Y, -0.1)],
             [(A.AUTOCONTRAST, 0), (A.EQUALIZE, 0), (A.TRANSLATE_X, 2)]]
    return ops + mixed


@pytest.mark.parametrize("kind", ["random", "constant", "two", "narrow"])
@pytest.mark.parametrize("flip", [False, True])
def test_forced_plans_every_op_at_extremes(kind, flip):
    rs = np.random.RandomState(5)
    H, W = 37, 53
    chains = _extreme_chains(H, W)
    imgs, plans = [], []
    for k, c in enumerate(chains):
        other = chains[(k * 7 + 3) % len(chains)]
        imgs.append(_image(rs, H, W, kind))
        plans.append(_plan([c, other, []], ws=rs.dirichlet([1.] * 3), m=rs.rand()))
    _check(imgs, plans, [flip] * len(imgs))


def test_random_plans_small_odd_sizes_and_ragged_batch():
    rs = np.random.RandomState(11)
    np.random.seed(3)
    imgs, plans, flips = [], [], []
    for k in range(48):
        H, W = [(7, 5), (13, 17), (31, 23), (9, 40), (64, 33)][k % 5]
        img = _image(rs, H, W, ["random", "two", "narrow"][k % 3])
        plan, _ = A.draw_plan(H, W, positional=bool(k & 1))
        imgs.append(img)
        plans.append(plan)
        flips.append(bool(k & 2))
    _check(imgs, plans, flips)


def test_batch_of_8_at_800x1333_ragged_and_repeatable():
    rs = np.random.RandomState(1)
    np.random.seed(17)
    sizes = [(800, 1333)] * 6 + [(800, 1201), (612, 800)]
    imgs, plans, flips = [], [], []
    for k, (H, W) in enumerate(sizes):
        imgs.append(_image(rs, H, W))
        plans.append(A.draw_plan(H, W, positional=k % 2 == 0)[0])
        flips.append(k % 3 == 0)
    got = _check(imgs, plans, flips)
    again = _check(imgs, plans, flips)
    for a, b in zip(got, again):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_staging_feeds_the_blur_the_host_path_images_and_train_step_is_finite(tmp_path, monkeypatch):
    """The loader's deferred plans through engine._to_device (side stream, as train_one_epoch stages them) equal the host path;
    then one train.main epoch step with --gpu_blur --expand_target_boxes and the three AugMix flags runs with finite losses."""
    from detectinblur_amd import engine, utils
    from detectinblur_amd import train as TR
    from detectinblur_amd.coco_utils import get_coco
    tf = TR.get_transform(True, blur=True, blur_ratio=1, non_pos_aug_mix=True, include_pos_aug_mix=True, aug_mix_target_expand=True,
                          defer_aug_mix=True)
    ds, _ = get_coco(None, "train", tf, synthetic=dict(num_images=4, size=(96, 131)))
    np.random.seed(1)
    random.seed(4)
    batch = utils.collate_fn([ds[i] for i in range(4)])
    images, targets, dicts = batch
    assert all(d["augmix"]["deferred"] for d in dicts)
    want = [A.apply_deferred_host(im, d["augmix"]).half() for im, d in zip(images, dicts)]
    staged = engine._to_device(list(images), copy.deepcopy(list(targets)), dicts, DEV, True, want_tables=True)
    torch.cuda.synchronize()
    for g, w in zip(staged[0], want):
        assert torch.equal(g.cpu().view(torch.int16), w.view(torch.int16))

    from tests.test_engine_ddp_cpu import _small_model
    monkeypatch.setattr(TR, "fasterrcnn_resnet50_fpn", lambda **kw: _small_model())
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    seen = []
    real = engine.train_one_epoch

    def spy(*a, **k):
        logger = real(*a, **k)
        seen.append({n: m.global_avg for n, m in logger.meters.items()})
        return logger
    monkeypatch.setattr(TR, "train_one_epoch", spy)
    argv = ["--synthetic", "--synthetic_images", "4", "--synthetic_size", "96", "131", "-b", "2", "--epochs", "1", "--blur_train",
            "--gpu_blur", "--expand_target_boxes", "--non_pos_aug_mix", "--include_pos_aug_mix", "--aug_mix_target_expand",
            "--output_dir", "", "--tensorboard_path", "", "--print_freq", "1", "--lr", "0.001"]
    TR.main(TR.build_parser().parse_args(argv))
    assert seen and all(np.isfinite(v) for v in seen[0].values() if isinstance(v, float)), seen
