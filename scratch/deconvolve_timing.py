"""--deconvolve_first on one MI355X: what profiles/deconvolve_first.txt records.

    python scratch/deconvolve_timing.py stage           the stage per 3 x 800 x 1333 Half image at N = 30 for a sweep PSF of each exposure end
                                                        (E = 1/25 and E = 1 at P = 0.001), against (a) the torch restatement on the GPU and
                                                        (b) 2 N launches of dib_sparse_blur in DIB_ACC_FP32 on the same image and table
    python scratch/deconvolve_timing.py cell [IMAGES]   sweep cell P2 E3 at 800 x 1333 (batch 1, graphed, IMAGES = 200 timed images): without the
                                                        stage, --deconvolve_first, --deblur_first --deblur_precision half, alternated three times
"""
import contextlib
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W, N = 800, 1333, 30


def sweep_psf(param, fraction, seed):
    """one PSF of the evaluation sweep, as transforms.BlurImage builds it (256 canvas, centred, the middle 128 x 128), uploaded as the
    engine uploads it"""
    from detectinblur_amd.transforms import make_psf
    np.random.seed(seed)
    return torch.HalfTensor(make_psf(param, fraction))


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stage(reps=7):
    from detectinblur_amd import _lib, blur_ops
    from detectinblur_amd.models import deconvolve as DC
    dev = torch.device("cuda:0")
    sharp = torch.rand(3, H, W, generator=torch.Generator().manual_seed(0)).half().to(dev)
    for label, fraction in (("E = 1/25", 1 / 25), ("E = 1", 1.0)):
        psf = sweep_psf(0.001, fraction, seed=1337).to(dev)
        tables = blur_ops.compact_psfs([psf], normalize=True)
        y = blur_ops.sparse_blur([sharp], [0], tables)[0]
        taps, segs = tables.header(0)[0], len(tables.segments(0))
        hip = lambda: DC.richardson_lucy_hip(y, tables, 0, N)                                  # noqa: E731
        blur = lambda: [blur_ops.sparse_blur([y], [0], tables, _lib.DIB_ACC_FP32) for _ in range(2 * N)]      # noqa: E731
        for fn in (hip, blur):
            fn()
        torch.cuda.synchronize()
        t_hip, t_blur = [], []
        for _ in range(reps):
            t_hip.append(_event_ms(hip))
            t_blur.append(_event_ms(blur))
        host_taps = DC.taps_of_table(tables, 0)
        ref = lambda: DC.richardson_lucy_torch(y, host_taps, N)                                # noqa: E731
        ref()
        t_ref = [_event_ms(ref) for _ in range(2)]
        err = float((hip() - ref()).abs().max())
        m_hip, m_blur, m_ref = np.median(t_hip), np.median(t_blur), np.median(t_ref)
        print("%-8s %4d taps, %3d segments: stage %.3f ms (min %.3f, max %.3f; %d runs) = %.1f us per sweep | (b) %d x dib_sparse_blur fp32 "
              "%.3f ms (min %.3f, max %.3f) = %.1f us per launch | (a) torch on the GPU %.1f ms | stage / (b) %.2f, (a) / stage %.0f | "
              "HIP against torch %.2e" % (label, taps, segs, m_hip, min(t_hip), max(t_hip), reps, 1e3 * m_hip / (2 * N), 2 * N, m_blur, min(t_blur),
                                          max(t_blur), 1e3 * m_blur / (2 * N), m_ref, m_hip / m_blur, m_ref / m_hip, err), flush=True)


def cell(n=200, passes=3, warm=8):
    from detectinblur_amd import evaluate as EV
    from detectinblur_amd import kernel_choices, train as TR, utils
    from detectinblur_amd.coco_utils import get_coco
    from detectinblur_amd.engine import evaluate
    from detectinblur_amd.models.deblur import Deblurer, write_random_checkpoint
    from detectinblur_amd.models.deconvolve import Deconvolver
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    kernel_choices.use_shipped_kernel_choices()
    dev = torch.device("cuda:0")
    d = tempfile.mkdtemp(prefix="dib_deconvolve_timing_")
    write_random_checkpoint(d, seed=0)
    with contextlib.redirect_stdout(io.StringIO()):
        deblurrer = Deblurer(d, dev, precision="half")
    TR.seed_everything(False)
    model = fasterrcnn_resnet50_fpn(num_classes=91, pretrained=False, pretrained_backbone=False).to(dev).eval()
    kinds = (("without", {}), ("deconvolve", dict(deconvolve_first=True, deconvolver=Deconvolver(N))),
             ("deblur half", dict(deblur_first=True, deblurer=deblurrer)))
    res = {k: [] for k, _ in kinds}
    for rep in range(passes + 1):                                      # pass 0 of each kind warms up (on fewer images)
        for name, kw in kinds:
            count = n if rep else 16
            tf = TR.get_transform(False, blur=True, blur_type=EV.SWEEP_PARAMS[1], blur_ratio=1, blur_exposure=EV.SWEEP_FRACTIONS[2])
            dset, _ = get_coco(None, "val", tf, synthetic=dict(num_images=warm + count, size=(H, W)))
            loader = torch.utils.data.DataLoader(dset, batch_size=1, shuffle=False, num_workers=4, collate_fn=utils.collate_fn, pin_memory=True)
            stamps = []

            def timed(it):
                for k, batch in enumerate(it):
                    if k == warm:
                        torch.cuda.synchronize()
                        stamps.append(time.perf_counter())
                    yield batch

            class L(object):
                dataset = dset

                def __iter__(self):
                    return timed(iter(loader))

                def __len__(self):
                    return len(loader)
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                evaluate(model, L(), device=dev, blurring_images=True, gpu_blur=True, expand_target_boxes=True, **kw)
            torch.cuda.synchronize()
            ips = count / (time.perf_counter() - stamps[0])
            print("pass %d %-12s %6.2f images/s (%d timed images after %d; whole pass %.1f s)" % (rep, name, ips, count, warm, time.perf_counter() - t0),
                  flush=True)
            if rep:
                res[name].append(ips)
    for name, _ in kinds:
        v = res[name]
        print("sweep cell P2 E3 at %d x %d, %-12s median %6.2f images/s (%s) = %.1f ms per image" % (H, W, name, np.median(v),
                                                                                                ", ".join("%.2f" % x for x in v), 1000 / np.median(v)))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "stage":
        stage()
    elif mode == "cell":
        cell(int(sys.argv[2]) if len(sys.argv) > 2 else 200)
    else:
        raise SystemExit(__doc__)
