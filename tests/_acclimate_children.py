"""Body of the `--acclimate_norm` detector test that needs a process of its own (tests/test_acclimate_norm_gpu.py), run through
the session's fork server as tests/_gpu_children.py's are: MIOpen's deterministic mode (without it the toy-size trunk is not
bit-reproducible: profiles/r4_nondeterminism.txt) must not write its kernel choices into the session's find-db copy."""
import os

from tests._gpu_children import _guarded

SIZE = ["--synthetic_size", "128", "160", "--min_size", "128", "--max_size", "160"]


def _state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items() if k.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked")}


def _same(a, b):
    import torch
    return sorted(a) == sorted(b) and all(a[k].shape == b[k].shape and torch.equal(a[k], b[k]) for k in a)


def _graph_and_pipeline():
    import tempfile
    os.environ["MIOPEN_USER_DB_PATH"] = tempfile.mkdtemp(prefix="dib_acclimate_miopen_")
    import contextlib
    import io
    import torch
    torch.backends.cudnn.deterministic = True
    from detectinblur_amd import evaluate, utils
    from detectinblur_amd.models.batchnorm import BatchNorm2d
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    out = {}

    # (1) the graphed trunk against eager inference: three images of one shape with changing content, every pass from the snapshot
    torch.manual_seed(0)
    m = fasterrcnn_resnet50_fpn(num_classes=91, pretrained=False, pretrained_backbone=False, min_size=128, max_size=160).cuda()
    m.roi_heads.score_thresh = 0.0                                   # a random-init head keeps detections to compare
    m = utils.convert_to_custom_batch_norm(m, batch_norm_to_use=BatchNorm2d)
    m = utils.set_batch_norm_acclimation_mode(utils.set_batch_momentum_zero(utils.set_batch_norm_N(m, 16)), True)
    m = utils.turn_batch_norm_on(utils.copy_BN_stats_to_old(m).eval())
    g = torch.Generator().manual_seed(3)
    imgs = [(torch.rand((3, 128, 160), generator=g) * (0.5 + 0.25 * k)).cuda() for k in range(3)]
    bns = [b for b in m.modules() if isinstance(b, BatchNorm2d)]

    def run(graphed):
        utils.restore_BN_stats_from_old(m)
        m.graph_inference = graphed
        for b in bns:
            b.last_path = None
        with torch.no_grad():
            dets = [{k: v.clone() for k, v in m([i.clone()])[0].items()} for i in imgs]
        torch.cuda.synchronize()
        return {"%d/%s" % (i, k): v for i, d in enumerate(dets) for k, v in d.items()}, _state(m)

    eager, eager_state = run(False)
    out["eager_paths"] = sorted({str(b.last_path) for b in bns})
    out["eager_reproducible"] = [_same(a, b) for a, b in zip((eager, eager_state), run(False))]
    first, first_state = run(True)                                   # image 0 eager, image 1 captured and replayed, image 2 replayed
    cache = m.__dict__.get("_trunk_graphs")
    out["captured"] = cache is not None and len(cache.graphs) == 1 and all(v is not None for v in cache.graphs.values())
    second, second_state = run(True)                                 # three replays
    out["graphed_equals_eager"] = [_same(first, eager), _same(first_state, eager_state), _same(second, eager), _same(second_state, eager_state)]
    out["counters"] = sorted({int(v) for k, v in eager_state.items() if k.endswith("num_batches_tracked")})
    out["detections"] = int(sum(v.shape[0] for k, v in eager.items() if k.endswith("scores")))
    out["images_differ"] = not torch.equal(eager["0/scores"][:8], eager["1/scores"][:8])
    del m

    # (2) engine.evaluate's pipelined loop against its plain loop, through the driver; and the synchronisations it counts
    syncs = [0]
    real_sync = torch.cuda.synchronize

    def counting(*a, **k):
        syncs[0] += 1
        return real_sync(*a, **k)

    def drive(extra, pipelined):
        seen = {}
        real = evaluate.evaluate

        def spy(model, loader, **kw):
            model.roi_heads.score_thresh = 0.0
            syncs[0] = 0
            torch.cuda.synchronize = counting
            try:
                seen["result"] = real(model, loader, **kw)
            finally:
                torch.cuda.synchronize = real_sync
            seen["syncs"] = syncs[0]
            seen["state"] = _state(model)
            seen["graphs"] = model.__dict__.get("_trunk_graphs")
            return seen["result"]

        if pipelined:
            os.environ.pop("DIB_NO_PIPELINE", None)
        else:
            os.environ["DIB_NO_PIPELINE"] = "1"
        evaluate.evaluate = spy
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                evaluate.main(evaluate.build_parser().parse_args(["--synthetic", "--synthetic_images", "3", "--vanilla_eval"] + SIZE + extra))
        finally:
            evaluate.evaluate = real
            os.environ.pop("DIB_NO_PIPELINE", None)
        dets = {"%d/%s" % (i, k): v for i, d in seen["result"]["detections"].items() for k, v in d.items()}
        return dets, seen

    plain, plain_seen = drive(["--acclimate_norm"], False)
    piped, piped_seen = drive(["--acclimate_norm"], True)
    frozen, frozen_seen = drive([], True)
    out["pipelined_equals_plain"] = [_same(piped, plain), _same(piped_seen["state"], plain_seen["state"])]
    out["pipelined_captured"] = piped_seen["graphs"] is not None and any(v is not None for v in piped_seen["graphs"].graphs.values())
    out["pipelined_counters"] = sorted({int(v) for k, v in piped_seen["state"].items() if k.endswith("num_batches_tracked")})
    out["pipelined_images"] = len(piped_seen["result"]["detections"])
    out["pipelined_detections"] = int(sum(v.shape[0] for k, v in piped.items() if k.endswith("scores")))
    out["syncs"] = {"acclimate": piped_seen["syncs"], "frozen": frozen_seen["syncs"]}
    out["frozen_differs"] = not _same(frozen, piped)
    return out


def graph_and_pipeline(out_path):
    _guarded(_graph_and_pipeline, out_path, ())
