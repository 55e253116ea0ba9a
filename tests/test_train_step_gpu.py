"""GPU integration: one blurred training step and one blurred evaluation pass through the engines
(`--blur_train --gpu_blur --expand_target_boxes`), exactly the call sequence of reference engine.py:74-158."""
import numpy as np
import pytest
import torch

import dib_oracle as O

pytestmark = pytest.mark.gpu


def _model():
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    torch.manual_seed(0)
    return fasterrcnn_resnet50_fpn(pretrained=False, pretrained_backbone=False, num_classes=91, min_size=160, max_size=224,
                                   rpn_pre_nms_top_n_train=400, rpn_post_nms_top_n_train=200, rpn_post_nms_top_n_test=100).cuda()


def _loader(train, n=4):
    import random
    from detectinblur_amd import utils
    from detectinblur_amd.coco_utils import SyntheticCocoDetection
    from detectinblur_amd.train import get_transform
    random.seed(3); np.random.seed(3)
    tf = get_transform(train, blur=True, blur_type=0.005, blur_ratio=1.0, low_exposure=True)
    ds = SyntheticCocoDetection(num_images=n, size=(150, 210), boxes_per_image=4, transforms=tf)
    return torch.utils.data.DataLoader(ds, batch_size=2 if train else 1, collate_fn=utils.collate_fn)


def test_blurred_train_step_and_eval():
    from detectinblur_amd.engine import evaluate, train_one_epoch
    m = _model()
    opt = torch.optim.SGD(m.parameters(), lr=0.002, momentum=0.9)
    w0 = m.backbone.body.conv1.weight.detach().clone()
    log = train_one_epoch(m, opt, _loader(True), torch.device("cuda"), epoch=0, print_freq=1, blur_train=True, gpu_blur=True,
                          expand_target_boxes=True, use_custom_image_norm=True, early_stop=None)
    assert log.meters["loss"].count == 2 and np.isfinite(log.meters["loss"].global_avg)
    assert not torch.equal(w0, m.backbone.body.conv1.weight.detach())
    out = evaluate(m, _loader(False), torch.device("cuda"), blurring_images=True, gpu_blur=True, expand_target_boxes=True)
    assert len(out["detections"]) == 4
    assert out["coco_stats"] is not None and len(out["coco_stats"]) == 12 and all(-1.0 <= v <= 1.0 for v in out["coco_stats"])


def test_engine_blur_equals_oracle_on_loader_batch():
    """What the engine feeds the detector is bit-identical to the oracle's blur of the same batch."""
    from detectinblur_amd import engine, utils
    from detectinblur_amd.models import blur_functions
    images_CPU, targets, blur_dicts = next(iter(_loader(True)))
    imgs, tg, psfs, *_ = engine._to_device(images_CPU, targets, blur_dicts, torch.device("cuda"), True)
    want_imgs = [i.half().numpy().copy() for i in images_CPU]
    want_psfs = [O.to_half_like_torch(bd["psf"]) for bd in blur_dicts]
    O.blur_image_list(want_imgs, blur_dicts, want_psfs)
    want_boxes = [O.expand_boxes(t["boxes"].numpy(), p, i.shape[1], i.shape[2]) for t, p, i in zip(targets, want_psfs, images_CPU)]
    blur_functions.blur_image_list(imgs, blur_dicts, psfs_GPU=psfs)
    tg = utils.expand_targets(tg, blur_dicts, psfs, imgs)
    for g, w in zip(imgs, want_imgs):
        assert np.array_equal(g.cpu().numpy().view(np.uint16), w.view(np.uint16))
    for t, w in zip(tg, want_boxes):
        assert np.array_equal(t["boxes"].cpu().numpy(), w)


def test_ensemble_routing_runs():
    from torch import nn
    from detectinblur_amd.engine import evaluate
    from detectinblur_amd.models.blur_estimator import resnet18
    nets = [_model() for _ in range(2)] * 2
    est = resnet18(); est.fc = nn.Linear(512, 4); est = est.cuda()
    out = evaluate(None, _loader(False, 2), torch.device("cuda"), blurring_images=True, gpu_blur=True, expand_target_boxes=True,
                   use_ensemble=True, ensemble_models=nets, blur_estimator=est, LEHE=True)
    assert len(out["routes"]) == 2 and all(r in (0, 1, 2, 3) for r in out["routes"])


def test_train_cli_with_stored_psfs_end_to_end(tmp_path, capsys):
    """BASELINE configs[3] in miniature: `train.py --blur_train --gpu_blur --use_stored_psfs` on a store
    written by the store builder (2 PSFs per directory), two iterations, finite losses, checkpoint saved."""
    from detectinblur_amd import train
    from detectinblur_amd.dataset_utils import generate_PSFs as G
    dest = str(tmp_path) + "/"
    G.main(G.get_parser().parse_args(["--destination_path", dest, "--num_workers", "1", "--total_num_psfs", "2", "--packed"]))
    out = str(tmp_path / "run")
    args = train.build_parser().parse_args([
        "--synthetic", "--synthetic_images", "4", "--synthetic_size", "160", "224", "--blur_train", "--gpu_blur",
        "--use_stored_psfs", "--stored_psf_directory", dest + "psfs", "--stored_psf_count", "2", "--param_index", "1",
        "--low_exposure", "--expand_target_boxes", "-b", "2", "--epochs", "1", "--early_stop", "2",
        "--lr", "0.002", "--print_freq", "1", "--output_dir", out, "--tensorboard_path", str(tmp_path / "tb")])
    # without --use_custom_image_norm: with stored PSFs the reference's blur dictionary carries param_index - 1 of the nearest-type
    # bin (transforms.py:427-428), here -1, for which get_norm_params keeps an all-zero std row (utils.py:219-273): the normalised
    # batch is inf / NaN in every pixel and the reference's step ends in "Loss is nan, stopping training" -- as this one does since
    # the trunk's fused ReLUs let a NaN through (tests/test_trunk_epilogue_f32_gpu.py)
    train.main(args)
    text = capsys.readouterr().out
    assert "loss_classifier" in text and "nan" not in text.lower().split("namespace")[-1]


def test_train_cli_with_stored_psfs_and_custom_norm_stops_at_the_nan_loss_like_the_reference(tmp_path, capsys):
    """The flags of the test above plus --use_custom_image_norm.  With stored PSFs the blur dictionary carries param_index - 1 of
    the nearest-type bin (reference transforms.py:427-428), here -1, for which get_norm_params keeps an all-zero std row (reference
    utils.py:249-268): every pixel of a blurred image is normalised to inf or NaN.  The reference's plain-torch trunk carries that to
    the loss and its loop stops at the step (engine.py:145-148); so does this one, now that the trunk's fused ReLUs let a NaN
    through -- with fmaxf(v, 0) they erased it and the run trained on with finite losses."""
    from detectinblur_amd import train, utils
    from detectinblur_amd.dataset_utils import generate_PSFs as G
    stds = utils.get_norm_params([{"blurring": True, "param_index": -1, "fraction_index": 1}], True)[1]
    assert (stds == 0).all()
    dest = str(tmp_path) + "/"
    G.main(G.get_parser().parse_args(["--destination_path", dest, "--num_workers", "1", "--total_num_psfs", "2", "--packed"]))
    args = train.build_parser().parse_args([
        "--synthetic", "--synthetic_images", "4", "--synthetic_size", "160", "224", "--blur_train", "--gpu_blur",
        "--use_stored_psfs", "--stored_psf_directory", dest + "psfs", "--stored_psf_count", "2", "--param_index", "1",
        "--low_exposure", "--expand_target_boxes", "--use_custom_image_norm", "-b", "2", "--epochs", "1", "--early_stop", "2",
        "--lr", "0.002", "--print_freq", "1", "--output_dir", str(tmp_path / "run"), "--tensorboard_path", str(tmp_path / "tb")])
    with pytest.raises(SystemExit) as stop:
        train.main(args)
    assert stop.value.code == 1
    assert "Loss is nan, stopping training" in capsys.readouterr().out


def test_evaluate_cli_ensemble_sweep_end_to_end(capsys, tmp_path):
    """BASELINE configs[4] in miniature: the (type x exposure) sweep through 4 detectors + estimator."""
    from detectinblur_amd import evaluate as E
    args = E.build_parser().parse_args(["--synthetic", "--synthetic_images", "2", "--synthetic_size", "160", "224", "--use_ensemble",
                                      "--LEHE", "--use_blur_estimator", "--blur_eval", "--gpu_blur", "--expand_target_boxes",
                                      "--early_stop", "1", "--tensorboard_path", str(tmp_path / "tb")])
    res = E.main(args)
    text = capsys.readouterr().out
    assert text.count("routes") == 15           # 3 blur types x 5 exposures
    assert len(res) == 15 and res["P1E0"].coco_eval["bbox"].stats.shape == (12,)
    from detectinblur_amd import tb_writer
    import os
    ev = os.path.join(str(tmp_path / "tb"), os.listdir(str(tmp_path / "tb"))[0])
    if not ev.endswith(".v2"):
        tags = {(t, s) for t, s, _ in tb_writer.read_scalars(ev)}
        assert ("P1/AccuraciesSweep", 1) in tags and ("P3/recall", 5) in tags      # reference evaluate.py:358-368


def test_train_cli_with_full_corruption_chain(tmp_path, capsys):
    """--add_noise --add_block --add_jpeg_artefacts behind the GPU blur, two iterations."""
    from detectinblur_amd import train
    args = train.build_parser().parse_args([
        "--synthetic", "--synthetic_images", "4", "--synthetic_size", "160", "224", "--blur_train", "--gpu_blur",
        "--param_index", "2", "--high_exposure", "--expand_target_boxes", "--add_noise", "--add_block", "--add_jpeg_artefacts",
        "-b", "2", "--epochs", "1", "--early_stop", "2", "--lr", "0.002", "--print_freq", "1", "--output_dir", str(tmp_path / "run"),
        "--tensorboard_path", str(tmp_path / "tb")])
    train.main(args)
    text = capsys.readouterr().out
    assert "loss_classifier" in text and "Loss is" not in text


def test_degenerate_boxes_raise_on_the_gpu_without_draining_the_queue():
    """The degenerate-box flag travels to pinned host memory behind the transform and is read at the end of forward
    (reference models/generalized_rcnn.py:119-129: same ValueError, same text)."""
    m = _model()
    m.train()
    imgs = [torch.rand(3, 150, 210, device="cuda"), torch.rand(3, 150, 210, device="cuda")]
    good = {"boxes": torch.tensor([[10., 20., 60., 70.]], device="cuda"), "labels": torch.tensor([3], device="cuda")}
    bad = {"boxes": torch.tensor([[5., 5., 50., 60.], [30., 40., 30., 90.]], device="cuda"), "labels": torch.tensor([1, 2], device="cuda")}
    means = np.tile([0.485, 0.456, 0.406], (2, 1)); stds = np.tile([0.229, 0.224, 0.225], (2, 1))
    with pytest.raises(ValueError, match=r"positive height and width. Found invaid box \[.*\] for target at index 1"):
        m(imgs, [good, bad], newMeans=means, newSTDs=stds)
    losses = m(imgs, [good, good], newMeans=means, newSTDs=stds)          # and the flag is clean again on the next call
    assert all(torch.isfinite(v) for v in losses.values())


def _full_model():
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    torch.manual_seed(0)
    return fasterrcnn_resnet50_fpn(pretrained=False, pretrained_backbone=False, num_classes=91).cuda().eval()


_MEANS = lambda n: np.tile([0.485, 0.456, 0.406], (n, 1))          # noqa: E731
_STDS = lambda n: np.tile([0.229, 0.224, 0.225], (n, 1))           # noqa: E731


def _det_equal(a, b):
    return all(torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in ("boxes", "labels", "scores"))


def test_graphed_inference_is_bit_reproducible_and_equals_eager_inference():
    """engine.evaluate runs the detector's static trunk (backbone + FPN + RPN head + proposal filtering) as a HIP graph per
    input shape: the recorded launches of the eager code.  At the evaluation sizes (min 800 / max 1333, batch 1: what the
    reference evaluates, evaluate.py:335-339) every kernel of the inference path is deterministic -- the two that were not,
    MIOpen's atomically accumulating kernels for the 16-channel RPN predictor and the strided downsample convolutions, are
    GEMMs in inference (profiles/r4_nondeterminism.txt) -- so: two replays on the same input are EQUAL, a replay equals the
    eager trunk, and graphed detections equal eager detections in full (boxes, labels, scores), for a shape that needs no
    resize, one that does (600 x 800 -> 800 x 1066, padded to 1088), a portrait one, repeated and interleaved."""
    m = _full_model()
    torch.manual_seed(1)
    images = [torch.rand(3, 800, 1333, device="cuda"), torch.rand(3, 600, 800, device="cuda"), torch.rand(3, 640, 480, device="cuda")]
    order = [0, 1, 0, 2, 1, 0, 2]
    with torch.no_grad():
        eager = [m([images[i]], newMeans=_MEANS(1), newSTDs=_STDS(1)) for i in order]
        eager2 = [m([images[i]], newMeans=_MEANS(1), newSTDs=_STDS(1)) for i in order]
        assert all(_det_equal(a, b) for a, b in zip(eager, eager2))                  # the eager path itself is reproducible
        m.graph_inference = True
        graphed = [m([images[i]], newMeans=_MEANS(1), newSTDs=_STDS(1)) for i in order]
        again = [m([images[i]], newMeans=_MEANS(1), newSTDs=_STDS(1)) for i in order]
        cache = m._trunk_graphs
        assert len(cache.graphs) == 3 and all(g is not None for g in cache.graphs.values())     # captured (2nd sighting), not eager
        assert len(eager[0][0]["boxes"]) > 0
        for e, g, a in zip(eager, graphed, again):
            assert _det_equal(e, g) and _det_equal(e, a)
        # the trunk itself: replay vs replay, replay vs the eager function, on the same padded batch
        for i in (0, 1):
            imgs, _ = m.transform([images[i]], None, _MEANS(1), _STDS(1))
            m._sizes[1].copy_(torch.tensor([[float(s[1]), float(s[0])] for s in imgs.image_sizes], device="cuda"))
            want = [t.clone() for t in m._trunk(imgs.tensors)]
            one = [t.clone() for t in cache(imgs.tensors)]
            two = [t.clone() for t in cache(imgs.tensors)]
            assert int(one[-2][0]) > 100                                               # proposals kept
            for w, a, b in zip(want, one, two):
                assert torch.equal(a, b)
                assert torch.equal(a, w)


def test_graphed_inference_follows_weight_updates():
    """A captured trunk reads the batch-norm folds through cached tensors (backbone._folded) and everything else through the
    live parameters.  After an optimizer step on EVERY parameter, after load_state_dict, and after the parameters moved to
    new storage, graphed inference equals eager inference with the current weights (the round-3 code replayed the folds of
    the first evaluation: train.py evaluates after every epoch)."""
    m = _model().eval()
    m.roi_heads.score_thresh = 0.0              # a perturbed random-init head keeps detections to compare
    torch.manual_seed(2)
    img = [torch.rand(3, 150, 210, device="cuda")]
    means, stds = _MEANS(1), _STDS(1)

    def both():
        with torch.no_grad():
            m.graph_inference = False
            e = m(list(img), newMeans=means, newSTDs=stds)
            m.graph_inference = True
            g = m(list(img), newMeans=means, newSTDs=stds)
            g = [{k: v.clone() for k, v in d.items()} for d in g]
        return e, g

    def close(e, g):
        # toy sizes: MIOpen's small-M kernels accumulate atomically (profiles/r4_nondeterminism.txt), so scores agree to ~1e-3 and
        # the detection count to a few; stale weights move scores by far more than that (checked below: > 1e-2)
        assert abs(len(e[0]["scores"]) - len(g[0]["scores"])) <= 5 and len(g[0]["scores"]) > 0
        k = min(5, len(e[0]["scores"]), len(g[0]["scores"]))
        assert torch.allclose(e[0]["scores"][:k], g[0]["scores"][:k], atol=2e-3), (e[0]["scores"][:k], g[0]["scores"][:k])

    both(); e0, g0 = both()                      # second sighting: captured
    assert len(m._trunk_graphs.graphs) == 1 and all(g is not None for g in m._trunk_graphs.graphs.values())
    close(e0, g0)
    graph = next(iter(m._trunk_graphs.graphs.values()))
    # (1) an optimizer step on every parameter (conv weights of the frozen-BN trunk included); the gradients are synthetic
    # (5 % of each tensor's mean magnitude): a real step on a random-init detector at this rate ends in NaNs
    opt = torch.optim.SGD(m.parameters(), lr=1.0)
    for p in m.parameters():
        p.grad = torch.randn_like(p) * 0.05 * p.detach().abs().mean().clamp(min=1e-3)
    opt.step()
    m.eval()
    e1, g1 = both()
    assert next(iter(m._trunk_graphs.graphs.values())) is graph          # same graph, refreshed folds
    close(e1, g1)
    assert not torch.allclose(e1[0]["scores"][:3], e0[0]["scores"][:3], atol=1e-2)      # the step did move the detector
    # (2) load_state_dict (in-place copies): back to a perturbed copy of the weights
    sd = {k: (v * 1.05 if v.is_floating_point() and "running_var" not in k else v) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    e2, g2 = both()
    assert next(iter(m._trunk_graphs.graphs.values())) is graph
    close(e2, g2)
    # (3) parameters on new storage: the old graphs hold dangling pointers and are dropped
    for p in m.backbone.parameters():
        p.data = p.data.clone()
    e3, g3 = both()
    assert graph not in list(m._trunk_graphs.graphs.values())
    both(); e4, g4 = both()
    assert len(m._trunk_graphs.graphs) == 1
    close(e4, g4)


def test_graph_cache_survives_more_shapes_than_it_holds():
    """Seven padded shapes through a cache of three graphs, revisited in an order that evicts and recaptures: every replay
    still equals the eager trunk -- in particular the anchors each graph reads (the generator keeps ONE geometry cached; the
    graph keeps its own alive) and the shared memory pool."""
    from detectinblur_amd.graphs import GraphCache
    m = _model().eval()
    m.__dict__["_trunk_graphs"] = GraphCache(m._trunk, limit=3, capture_after=1)
    m.roi_heads.score_thresh = 0.0
    torch.manual_seed(3)
    shapes = [(150, 210), (120, 224), (160, 160), (100, 224), (130, 200), (160, 224), (224, 140)]
    imgs = [torch.rand(3, h, w, device="cuda") for h, w in shapes]
    visit = [0, 1, 2, 3, 0, 4, 5, 1, 6, 0, 2, 3, 6, 5]
    with torch.no_grad():
        for i in visit:
            m.graph_inference = True
            g = m([imgs[i]], newMeans=_MEANS(1), newSTDs=_STDS(1))
            g = [{k: v.clone() for k, v in d.items()} for d in g]
            m.graph_inference = False
            e = m([imgs[i]], newMeans=_MEANS(1), newSTDs=_STDS(1))
            assert abs(len(e[0]["scores"]) - len(g[0]["scores"])) <= 5 and len(g[0]["scores"]) > 0, i
            k = min(5, len(e[0]["scores"]), len(g[0]["scores"]))
            assert torch.allclose(e[0]["scores"][:k], g[0]["scores"][:k], atol=2e-4), i
            assert torch.allclose(e[0]["boxes"][:k], g[0]["boxes"][:k], atol=0.5), i
    assert len(m._trunk_graphs.graphs) == 3
