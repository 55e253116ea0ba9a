"""Detection overlays on the GPU: device time of the dib_overlay_rgb8 launch and the cost of saving pictures in a sweep cell
(profiles/detection_overlay.txt).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/k -o ov -- python scratch/overlay_timing.py kernel
    python scratch/overlay_timing.py report OUT/k/ov_kernel_trace.csv
    python scratch/overlay_timing.py cell [images] [workers]

`kernel`: one 3 x 800 x 1333 Half image, one call = one image = one launch, with 0, 10 and 100 boxes (seeded, all drawn): 5 warm-up
calls and 50 timed ones per box count (the trace's sections are told apart by their order, 55 launches each).  Also prints the time
per call from device events around the 50 calls.
`report`: the launches' device times from the trace, per section, against the byte floor (6 B in + 3 B out per pixel at 8 TB/s).
`cell`: engine.evaluate as the sweep calls it (P1E1, --gpu_blur --expand_target_boxes, Faster R-CNN random init, synthetic
800 x 1333 images through the loader), `images` timed images after 8, in three modes alternated three times:
    off      no image_output_folder
    this     image_output_folder: HIP render + PngWriter (4 worker threads)
    inline   image_output_folder, with the render and the writer replaced by the reference's shape: `.float().cpu()`, render_host and
             PIL's save inside the loop, nothing overlapped
"""
import contextlib
import csv
import io
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from detectinblur_amd import overlay  # noqa: E402

H, W = 800, 1333
BOX_COUNTS = (0, 10, 100)
WARM, TIMED = 5, 50


def _detection(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(n, 2, generator=g) * torch.tensor([W - 100.0, H - 100.0])
    wh = 32 + torch.rand(n, 2, generator=g) * 368                     # the synthetic dataset's box sizes
    return {"boxes": torch.cat([xy, xy + wh], dim=1), "labels": torch.randint(1, 91, (n,), generator=g)}


def kernel():
    dev = torch.device("cuda:0")
    image = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)).half().to(dev)
    for n in BOX_COUNTS:
        det = _detection(n)
        for _ in range(WARM):
            overlay.render_device([image], [det])
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(TIMED):
            overlay.render_device([image], [det])
        b.record()
        torch.cuda.synchronize()
        print("%3d boxes: %.1f us per call between device events (%d calls: plan upload, launch and the allocator included)"
              % (n, a.elapsed_time(b) * 1e3 / TIMED, TIMED))


def report(path):
    rows = [r for r in csv.DictReader(open(path)) if "overlay_rgb8" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = WARM + TIMED
    assert len(rows) == per * len(BOX_COUNTS), len(rows)
    floor = H * W * 9 / 8e12 * 1e6
    print("dib_overlay_rgb8, 3 x %d x %d Half, device time per launch from the kernel trace (%d timed launches behind %d); byte floor "
          "%.2f us (%.1f MB at 8 TB/s)" % (H, W, TIMED, WARM, floor, H * W * 9 / 1e6))
    for k, n in enumerate(BOX_COUNTS):
        t = np.array([int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows[k * per + WARM:(k + 1) * per]]) / 1e3
        print("%3d boxes: median %.2f us, min %.2f us, max %.2f us  (%.2f TB/s at the median, %.1fx the floor)"
              % (n, np.median(t), t.min(), t.max(), H * W * 9 / np.median(t) / 1e6, np.median(t) / floor))


class _Timed(object):
    """A loader that stamps the clock in front of batch `warm`."""

    def __init__(self, loader, warm, dataset):
        self.loader, self.warm, self.stamps, self.dataset = loader, warm, [], dataset

    def __iter__(self):
        for k, batch in enumerate(iter(self.loader)):
            if k == self.warm:
                torch.cuda.synchronize()
                self.stamps.append(time.perf_counter())
            yield batch

    def __len__(self):
        return len(self.loader)


@contextlib.contextmanager
def _inline_host_path():
    """The reference's shape inside the same loop: the picture is fetched, drawn and encoded where the detections arrive."""
    render, submit = overlay.render_device, overlay.PngWriter.submit
    overlay.render_device = lambda images, detections, stream=None: [(images[0], detections[0])]

    def inline(self, index, picture):
        image, det = picture
        overlay.save_png(self.path(index), overlay.render_host(image.float().cpu(), det["boxes"], det["labels"], det.get("scores")))
    overlay.PngWriter.submit = inline
    try:
        yield
    finally:
        overlay.render_device, overlay.PngWriter.submit = render, submit


def cell(n=200, workers=8):
    from detectinblur_amd import evaluate as EV
    from detectinblur_amd import kernel_choices, utils
    from detectinblur_amd import train as TR
    from detectinblur_amd.coco_utils import get_coco
    from detectinblur_amd.engine import evaluate
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    ctx = utils.loader_context() if workers else None
    kernel_choices.use_shipped_kernel_choices()
    TR.seed_everything(False)
    dev = torch.device("cuda:0")
    model = fasterrcnn_resnet50_fpn(num_classes=91, pretrained=False, pretrained_backbone=False).to(dev).eval()
    warm = 8
    root = tempfile.mkdtemp(prefix="dib_overlay_timing_")
    rates = {"off": [], "this": [], "inline": []}
    try:
        for rep in range(-1, 3):                                      # rep -1: a short untimed pass (graph capture, kernel choices)
            for mode in ("off", "this", "inline"):
                count = warm + (n if rep >= 0 else 8)
                with contextlib.redirect_stdout(io.StringIO()):
                    tf = TR.get_transform(False, blur=True, blur_type=EV.SWEEP_PARAMS[0], blur_ratio=1, blur_exposure=EV.SWEEP_FRACTIONS[0])
                    ds, _ = get_coco(None, "val", tf, synthetic=dict(num_images=count, size=(H, W)))
                loader = _Timed(torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, num_workers=workers, collate_fn=utils.collate_fn,
                                                            pin_memory=True, multiprocessing_context=ctx), warm, ds)
                folder = None if mode == "off" else os.path.join(root, "%s_%d" % (mode, rep))
                with contextlib.redirect_stdout(io.StringIO()), (_inline_host_path() if mode == "inline" else contextlib.nullcontext()):
                    out = evaluate(model, loader, device=dev, blurring_images=True, gpu_blur=True, expand_target_boxes=True,
                                   image_output_folder=folder)
                torch.cuda.synchronize()
                took = time.perf_counter() - loader.stamps[0]
                if folder is not None:
                    files = os.listdir(folder)
                    assert len(files) == count, (len(files), count)
                    size = sum(os.path.getsize(os.path.join(folder, f)) for f in files) / len(files)
                    shutil.rmtree(folder)
                if rep < 0:
                    continue
                rates[mode].append(n / took)
                drawn = sum(int((d["scores"] > 0.5).sum()) for d in out["detections"].values())
                print("rep %d  %-6s %6.1f images/s  (%d images after %d; %d boxes above 0.5 drawn%s)"
                      % (rep, mode, n / took, n, warm, drawn, "" if folder is None else "; %.2f MB per PNG" % (size / 1e6)), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    for mode in ("off", "this", "inline"):
        print("median %-6s %6.1f images/s  runs %s" % (mode, float(np.median(rates[mode])), ", ".join("%.1f" % r for r in rates[mode])))
    print("this path is %s than the inline host path in this collection (%.1f vs %.1f images/s)"
          % ("NOT SLOWER" if np.median(rates["this"]) >= np.median(rates["inline"]) else "SLOWER", np.median(rates["this"]), np.median(rates["inline"])))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "kernel":
        kernel()
    elif mode == "report":
        report(sys.argv[2])
    elif mode == "cell":
        cell(*[int(a) for a in sys.argv[2:4]])
    else:
        raise SystemExit(__doc__)
