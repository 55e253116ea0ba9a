"""Body of the `--restoration_metrics` driver test that needs processes of its own (tests/test_restoration_metrics_gpu.py), run through
the session's fork server as tests/_gpu_children.py's are: DIB_NO_PIPELINE=1 must not leak into the test session, and each run builds
its detector and its trunk graph from scratch."""
import os

from tests._gpu_children import _guarded


def _one_cell(argv, no_pipeline):
    """`evaluate.main(argv)` restricted to one cell of the sweep (P1, the third exposure), in this (fresh) process: the cell's restoration
    figures as the exact hex form of their doubles, a SHA-256 over every detection, and how many images went through the split (pipelined) forward pass"""
    import contextlib
    import hashlib
    import io
    import numpy as np
    if no_pipeline:
        os.environ["DIB_NO_PIPELINE"] = "1"
    else:
        os.environ.pop("DIB_NO_PIPELINE", None)
    os.environ.pop("DIB_NO_GRAPHS", None)
    import torch
    torch.backends.cudnn.deterministic = True                # MIOpen's atomics-free kernels: detections comparable across processes
    from detectinblur_amd import evaluate
    from detectinblur_amd.models.generalized_rcnn import GeneralizedRCNN
    evaluate.SWEEP_PARAMS = evaluate.SWEEP_PARAMS[:1]
    evaluate.SWEEP_FRACTIONS = evaluate.SWEEP_FRACTIONS[2:3]
    build = evaluate.fasterrcnn_resnet50_fpn                 # a random-init head scores every class near 1 / 91: keep its detections, so
    evaluate.fasterrcnn_resnet50_fpn = lambda *a, **k: build(*a, **dict(k, box_score_thresh=0.0))      # that they depend on the image
    split = [0]
    real = GeneralizedRCNN.launch_trunk

    def counted(self, *a, **k):
        handle = real(self, *a, **k)
        split[0] += handle is not None
        return handle
    GeneralizedRCNN.launch_trunk = counted
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = evaluate.main(evaluate.build_parser().parse_args(list(argv)))
    assert len(res) == 1, sorted(res)
    r = list(res.values())[0]
    h = hashlib.sha256()
    for k in sorted(r["detections"]):
        h.update(np.int64(k).tobytes())
        for f in ("boxes", "scores", "labels"):
            h.update(np.ascontiguousarray(r["detections"][k][f].numpy()).tobytes())
    out = {"images": len(r["detections"]), "boxes": int(sum(len(d["boxes"]) for d in r["detections"].values())), "sha256": h.hexdigest(),
           "split_forward_passes": split[0], "has_key": "restoration" in r,
           "lines": [l for l in buf.getvalue().splitlines() if "Restoration" in l]}
    if "restoration" in r:
        rest = r["restoration"]
        out["restoration"] = {name: ({k: float(v).hex() for k, v in val.items()} if isinstance(val, dict) else
                                     (float(val).hex() if isinstance(val, float) else val)) for name, val in rest.items()}
    return out


def one_cell(out_path, argv, no_pipeline):
    _guarded(_one_cell, out_path, (argv, no_pipeline))
