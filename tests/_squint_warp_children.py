"""Body of the squint-warp detector tests that needs a process of its own (tests/test_squint_warp_gpu.py), run through the
session's fork server as tests/_gpu_children.py's are: DIB_NO_FUSED_WARP=1 must not leak into the test session, and MIOpen's
deterministic mode (without it the toy-size trunk is not bit-reproducible: profiles/r4_nondeterminism.txt) must not write its
kernel choices into the session's find-db copy."""
import os

from tests._gpu_children import _guarded


def toy_detector(seed=0):
    import torch
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    torch.manual_seed(seed)
    return fasterrcnn_resnet50_fpn(num_classes=5, pretrained=False, pretrained_backbone=False, warp_internally=True, min_size=96,
                                   max_size=128).cuda()


def toy_batch(dev="cuda"):
    import torch
    g = torch.Generator().manual_seed(11)
    imgs = [torch.rand(3, 96, 128, generator=g).to(dev), torch.rand(3, 90, 120, generator=g).to(dev)]
    tg = [{"boxes": torch.tensor([[10.0, 12, 60, 70]], device=dev), "labels": torch.tensor([2], device=dev)},
          {"boxes": torch.tensor([[5.0, 8, 40, 44], [30, 30, 80, 85]], device=dev), "labels": torch.tensor([1, 3], device=dev)}]
    params = (torch.tensor([0.4, -0.2]).half().to(dev), torch.tensor([0.9, 0.85]).half().to(dev), torch.tensor([1.0, 0.97]).half().to(dev))
    return imgs, tg, params


def _det_equal(a, b):
    import torch
    return all(x[k].shape == y[k].shape and torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in ("boxes", "labels", "scores"))


def _detector_without_fused_warp_then_graphed():
    import detectinblur_amd
    detectinblur_amd.use_shipped_kernel_choices()           # a private copy of the shipped find-db, as the test session has
    import torch
    out = {}
    # (1) which trunk parameters the torch-path warper hands a gradient to
    os.environ["DIB_NO_FUSED_WARP"] = "1"
    m = toy_detector().train()
    imgs, tg, (th, l1, l2) = toy_batch()
    assert not m.warper.takes_fused(torch.zeros(1, 3, 4, 4, device="cuda"))
    sum(m(imgs, tg, thetas=th, lambda1s=l1, lambda2s=l2).values()).backward()
    out["trunk_grads_torch_path"] = sorted(n for n, p in m.backbone.named_parameters() if p.grad is not None)
    del os.environ["DIB_NO_FUSED_WARP"]
    # (2) the graphed warped trunk against eager inference, for three (theta, l1, l2), in MIOpen's deterministic mode
    torch.backends.cudnn.deterministic = True
    m = toy_detector().eval()
    m.roi_heads.score_thresh = 0.0                           # a random-init head keeps detections to compare
    sets = [(th, l1, l2),
            (torch.tensor([1.1, 0.6]).half().cuda(), torch.tensor([0.8, 1.0]).half().cuda(), torch.tensor([0.95, 0.75]).half().cuda()),
            (torch.tensor([-0.7, 2.0]).half().cuda(), torch.tensor([1.0, 0.7]).half().cuda(), torch.tensor([0.85, 0.9]).half().cuda())]

    def run(graphed, p):
        m.graph_inference = graphed
        with torch.no_grad():
            d = m([i.clone() for i in imgs], thetas=p[0], lambda1s=p[1], lambda2s=p[2])
        return [{k: v.clone() for k, v in x.items()} for x in d]

    eager = [run(False, p) for p in sets]
    out["eager_reproducible"] = all(_det_equal(a, run(False, p)) for a, p in zip(eager, sets))
    run(True, sets[0]); first = run(True, sets[0])           # second sighting: captured
    cache = m.__dict__.get("_warped_trunk_graphs")
    out["captured"] = cache is not None and len(cache.graphs) == 1 and all(g is not None for g in cache.graphs.values())
    out["plain_trunk_cache_used"] = "_trunk_graphs" in m.__dict__
    replays = [first, run(True, sets[1]), run(True, sets[2]), run(True, sets[0])]
    out["still_one_graph"] = cache is not None and len(cache.graphs) == 1
    out["replay_equals_eager"] = [_det_equal(r, eager[i]) for r, i in zip(replays, (0, 1, 2, 0))]
    out["detections"] = [int(sum(len(d["scores"]) for d in e)) for e in eager]
    out["sets_differ"] = [not _det_equal(eager[a], eager[b]) for a, b in ((0, 1), (0, 2), (1, 2))]
    return out


def detector_without_fused_warp_then_graphed(out_path):
    _guarded(_detector_without_fused_warp_then_graphed, out_path, ())
