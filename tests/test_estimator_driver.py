"""The estimator driver's command line (reference train_blur_estimator.py:511-585, flag for flag), what the new flags do on the
CPU -- aspect-ratio batches, deferred AugMix plans through the estimator's staging, TensorBoard scalars, --pretrained from the local
cache only -- and the one piece of arithmetic the fused input batch leans on that needs no GPU to check."""
import contextlib
import copy
import io
import os
import random

import numpy as np
import pytest
import torch

import pin_inputs as PI
from detectinblur_amd import engine_blur_estimator as EB
from detectinblur_amd import tb_writer
from detectinblur_amd import train_blur_estimator as TB
from detectinblur_amd import transforms as T

# flag names of reference train_blur_estimator.py:511-585
REFERENCE_FLAGS = ["--dataset", "--data_path", "--aspect-ratio-group-factor", "--use_stored_psfs", "--stored_psf_directory", "--crop_images",
                   "--resize_images", "--quantize_image", "--model", "--trainable_backbone_blocks", "--pretrained", "--device", "-b",
                   "--batch_size", "-j", "--workers", "--lr", "--lr-step-size", "--lr-steps", "--lr-gamma", "--epochs", "--momentum",
                   "--resume", "--start_from_weights", "--start_epoch", "--early_stop", "--eval_first", "--test_only", "--wd",
                   "--weight-decay", "--tensorboard_path", "--output_dir", "--image_output_dir", "--blur_train", "--cpu_blur", "--gpu_blur",
                   "--param_index", "--LEHE_blur_seg", "--high_exposure", "--low_exposure", "--expand_target_boxes", "--dont_center_psf",
                   "--add_noise", "--noise_level", "--add_block", "--add_jpeg_artefacts", "--non_pos_aug_mix", "--include_pos_aug_mix",
                   "--aug_mix_target_expand", "--world-size", "--dist-url"]
# the reference's defaults (its two machine paths, --data_path and --stored_psf_directory, are not defaults anyone else can use)
REFERENCE_DEFAULTS = dict(dataset="coco", aspect_ratio_group_factor=3, use_stored_psfs=False, crop_images=False, resize_images=False,
                          quantize_image=False, model="fasterrcnn_resnet50_fpn", trainable_backbone_blocks=3, pretrained=False,
                          device="cuda", batch_size=8, workers=0, lr=0.04, lr_step_size=8, lr_steps=[16, 22], lr_gamma=0.1, epochs=37,
                          momentum=0.9, resume=None, start_from_weights=None, start_epoch=0, early_stop=None, eval_first=False,
                          test_only=False, weight_decay=1e-4, tensorboard_path="debug", output_dir="debug", image_output_dir="debug",
                          blur_train=False, cpu_blur=False, gpu_blur=False, param_index=None, LEHE_blur_seg=False, high_exposure=False,
                          low_exposure=False, expand_target_boxes=False, dont_center_psf=False, add_noise=False, noise_level=0.001,
                          add_block=False, add_jpeg_artefacts=False, non_pos_aug_mix=False, include_pos_aug_mix=False,
                          aug_mix_target_expand=False, world_size=1, dist_url="env://")


def test_every_reference_flag_is_accepted_with_its_default():
    parser = TB.build_parser()
    known = {s for a in parser._actions for s in a.option_strings}
    assert not [f for f in REFERENCE_FLAGS if f not in known]
    d = vars(parser.parse_args([]))
    assert {k: d.get(k, "<absent>") for k in REFERENCE_DEFAULTS} == REFERENCE_DEFAULTS
    # this repo's additions stay
    assert {"--synthetic", "--synthetic_images", "--synthetic_size", "--stored_psf_count", "--blur_acc_mode"} <= known
    # the flags the reference parses and never reads say so
    for a in parser._actions:
        if a.dest in ("model", "trainable_backbone_blocks", "lr_step_size", "image_output_dir", "expand_target_boxes"):
            assert "never read" in a.help, a.dest
    assert "not offered" not in TB.__doc__


def test_grouped_sampler_on_one_shape_yields_the_plain_batches():
    """--aspect-ratio-group-factor 3 (the new default) on a dataset of one image shape -- every synthetic run, every existing test --
    batches exactly as BatchSampler(drop_last=True) did."""
    from detectinblur_amd.coco_utils import get_coco
    from detectinblur_amd.group_by_aspect_ratio import GroupedBatchSampler, create_aspect_ratio_groups
    from detectinblur_amd.train import get_transform
    dataset, _ = get_coco(None, "train", get_transform(True), synthetic=dict(num_images=23, size=(48, 64)), with_masks=False)
    with contextlib.redirect_stdout(io.StringIO()):
        groups = create_aspect_ratio_groups(dataset, k=3)
    assert len(set(groups)) == 1
    for batch_size in (2, 4, 5):
        def sampler():
            return torch.utils.data.RandomSampler(dataset, generator=torch.Generator().manual_seed(77))
        grouped = [list(b) for b in GroupedBatchSampler(sampler(), groups, batch_size)]
        plain = [list(b) for b in torch.utils.data.BatchSampler(sampler(), batch_size, drop_last=True)]
        assert grouped == plain and len(plain) == 23 // batch_size
        assert len(GroupedBatchSampler(sampler(), groups, batch_size)) == len(plain)


# ---- deferred AugMix plans through the estimator's staging ------------------------------------------------------------------

def _augmix_loader(defer):
    """3 batches x 2 images of 48 x 64, AugMix (positional ops included) -> ToTensor -> flip, the pixels of AugMix either applied
    here (`defer` False: the reference's loader) or left as a plan in blur_dict["augmix"]."""
    tf = T.Compose([T.AugMix(include_pos_aug_mix=True, defer=defer), T.ToTensor(), T.RandomHorizontalFlip(0.5)])
    rs = np.random.RandomState(31)
    random.seed(5)
    np.random.seed(5)
    loader = PI.ListLoader()
    flips = 0
    for k in range(3):
        images, targets, dicts = [], [], []
        for j in range(2):
            image = torch.from_numpy(rs.randint(0, 256, (3, 48, 64)).astype(np.float32) / np.float32(255))
            target = {"boxes": torch.tensor([[4.0, 5.0, 30.0 + j, 40.0 - k]]), "labels": torch.tensor([1 + j])}
            image, target, bd = tf(image, target, {"blurring": bool((k + j) % 2), "param_index": k % 3, "fraction_index": (k + 2 * j) % 5,
                                                   "psf": [0]})
            flips += bool(bd["augmix"]["flip"])
            assert bd["augmix"]["deferred"] is defer
            images.append(image); targets.append(target); dicts.append(bd)
        loader.append((tuple(images), tuple(targets), tuple(dicts)))
    loader.dataset = object()
    return loader, flips


def _train(loader):
    torch.manual_seed(0)
    np.random.seed(0)
    model = PI.ToyClassifier(16, 1)
    opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9)
    criterion, losses = torch.nn.CrossEntropyLoss(), []

    def crit(output, target):
        loss = criterion(output, target)
        losses.append(float(loss.detach()))
        return loss
    with contextlib.redirect_stdout(io.StringIO()):
        EB.train_one_epoch(model, opt, crit, loader, torch.device("cpu"), print_freq=1)
    return losses, {k: v.clone() for k, v in model.state_dict().items()}


def test_deferred_augmix_plans_are_applied_by_the_estimators_staging_cpu():
    deferred, flips = _augmix_loader(True)
    applied, _ = _augmix_loader(False)
    assert 0 < flips < 6                                        # mirrored and unmirrored plans
    from detectinblur_amd import augmix
    ops = {op for _, _, dicts in deferred for bd in dicts for chain in bd["augmix"]["chains"] for op, _ in chain}
    assert ops & set(augmix.POSITIONAL_OPS) and ops - set(augmix.POSITIONAL_OPS)      # positional and non-positional chains
    # the loaders differ: the deferred one still holds the unaugmented pixels
    assert not all(torch.equal(a, b) for (ia, _, _), (ib, _, _) in zip(deferred, applied) for a, b in zip(ia, ib))
    snapshot = copy.deepcopy([bd for _, _, dicts in deferred for bd in dicts])
    want_losses, want_weights = _train(applied)
    got_losses, got_weights = _train(deferred)
    assert len(got_losses) == 3 and got_losses == want_losses
    for k in want_weights:
        assert torch.equal(got_weights[k], want_weights[k]), k
    assert [bd["augmix"]["flip"] for _, _, dicts in deferred for bd in dicts] == [bd["augmix"]["flip"] for bd in snapshot]


# ---- the driver ------------------------------------------------------------------------------------------------------------------

_RUN = ["--synthetic", "--synthetic_size", "64", "96", "--device", "cpu", "--cpu_blur", "--blur_train",
        "--non_pos_aug_mix", "--include_pos_aug_mix", "-b", "2", "--epochs", "1", "--early_stop", "1", "--print_freq", "1"]
TAGS = {"losses/loss", "losses/overallLoss", "learningRate", "Blurred/Top1Accuracy", "Blurred/Top2Accuracy"}


def _events(path):
    return [os.path.join(path, f) for f in os.listdir(path) if f.startswith("events.out.tfevents.")] if os.path.isdir(path) else []


def test_driver_runs_with_augmix_cpu_blur_and_tensorboard(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    n_threads = torch.get_num_threads()
    try:
        with contextlib.redirect_stdout(io.StringIO()) as out:
            TB.main(TB.build_parser().parse_args(_RUN + ["--tensorboard_path", str(tmp_path / "tb"), "--output_dir", str(tmp_path / "w")]))
        assert "Top 1 Accuracy" in out.getvalue()
        assert (tmp_path / "w" / "blur_estimator_0.pth").exists()
        files = _events(str(tmp_path / "tb"))
        assert len(files) == 1
        scalars = tb_writer.read_scalars(files[0])
        assert TAGS <= {tag for tag, _, _ in scalars}
        top = {tag: (step, value) for tag, step, value in scalars if tag.startswith("Blurred/")}
        assert all(step == 0 and 0.0 <= value <= 100.0 for step, value in top.values())
        assert top["Blurred/Top2Accuracy"][1] >= top["Blurred/Top1Accuracy"][1]
        # an empty path: no writer, no event file anywhere under the working directory
        with contextlib.redirect_stdout(io.StringIO()):
            TB.main(TB.build_parser().parse_args(_RUN[:-4] + ["--early_stop", "0", "--tensorboard_path", "", "--output_dir", ""]))
        found = [os.path.join(d, f) for d, _, fs in os.walk(str(tmp_path)) for f in fs if f.startswith("events.out.tfevents.")]
        assert found == files
    finally:
        torch.set_num_threads(n_threads)


def test_pretrained_without_a_cached_file_raises_and_fetches_nothing(tmp_path, monkeypatch):
    import urllib.request
    from detectinblur_amd.models import blur_estimator, faster_rcnn

    def no_network(*a, **k):
        raise AssertionError("--pretrained must never reach for the network")
    monkeypatch.setattr(urllib.request, "urlopen", no_network)
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", no_network)
    monkeypatch.setattr(torch.hub, "download_url_to_file", no_network)
    monkeypatch.setenv("DIB_WEIGHTS_DIR", str(tmp_path / "none"))
    monkeypatch.setenv("TORCH_HOME", str(tmp_path / "torch_home"))
    monkeypatch.chdir(tmp_path)
    assert faster_rcnn.find_pretrained("resnet18") is None
    with pytest.raises(RuntimeError, match="cannot be downloaded here"):
        blur_estimator.resnet18(pretrained=True)
    with pytest.raises(RuntimeError, match="resnet18-"), contextlib.redirect_stdout(io.StringIO()):
        TB.main(TB.build_parser().parse_args(_RUN + ["--pretrained", "--tensorboard_path", "", "--output_dir", ""]))
    # a cached file is found and loaded: torchvision's key layout is this model's
    os.makedirs(str(tmp_path / "weights"))
    torch.manual_seed(3)
    donor = blur_estimator.resnet18()
    torch.save(donor.state_dict(), str(tmp_path / "weights" / faster_rcnn.PRETRAINED_FILES["resnet18"][0]))
    loaded = blur_estimator.resnet18(pretrained=True)
    assert all(torch.equal(v, donor.state_dict()[k]) for k, v in loaded.state_dict().items())


def test_quantise_division_and_reciprocal_multiply_round_to_the_same_half():
    """DIB_EPILOGUE_QUANTIZE divides, float(k) / 255.f (include/dib.h); ATen's device kernel for `half_tensor / 255` multiplies by
    float(1) / 255.f.  For the 256 integers a uint8 holds both round to the same Half: k / 255 is never closer than 2^-20 (relative)
    to a midpoint between two Halves, and the reciprocal's error is below 2^-23."""
    k = np.arange(256, dtype=np.float32)
    divided = (k / np.float32(255)).astype(np.float16)
    multiplied = (k * (np.float32(1) / np.float32(255))).astype(np.float16)
    assert np.array_equal(divided.view(np.uint16), multiplied.view(np.uint16))
    assert np.array_equal(divided.view(np.uint16), (torch.arange(256, dtype=torch.uint8).type(torch.half) / 255).numpy().view(np.uint16))
