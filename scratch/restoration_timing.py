"""The figures of profiles/restoration_sweep.txt (one MI355X).

    python scratch/restoration_timing.py call           device time of one K = 2 restoration_quality call with its accumulator against the two
                                                        psnr_ssim_hip calls it replaces (and one of them), event pairs, 5 alternated rounds of
                                                        20 calls, at 3 x 800 x 1333 and 3 x 128 x 160
    python scratch/restoration_timing.py cell [IMAGES]  sweep cell P2 E3 at 800 x 1333 (batch 1, graphed, IMAGES = 200 timed images) with
                                                        --deconvolve_first: without and with --restoration_metrics, alternated three times
DIB_HIP_LIB selects another build of the library (csrc: `make ... HIPFLAGS+=-DDIB_RQ_RESIDENT` for the tile kernel that keeps all eight
row-sum planes resident)."""
import contextlib
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W, N = 800, 1333, 30


def timed(fn, n=20):
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return ts


def call():
    from detectinblur_amd import quality as Q
    dev = torch.device("cuda", 0)
    for shape in ((3, H, W), (3, 128, 160)):
        g = torch.Generator().manual_seed(0)
        ref = torch.rand(shape, generator=g).half().to(dev)
        blurred = (0.6 * ref + 0.4 * ref.roll(3, 2)).half()
        restored = 0.9 * ref.float() + 0.1 * ref.float().roll(1, 2)
        out2, acc = torch.zeros(6, device=dev), torch.zeros(12, dtype=torch.float64, device=dev)
        work2 = torch.empty(Q.restoration_workspace_bytes(2, *shape) // 8, dtype=torch.float64, device=dev)
        oa, ob = torch.zeros(3, device=dev), torch.zeros(3, device=dev)
        wa = torch.empty(Q.workspace_bytes(*shape) // 8, dtype=torch.float64, device=dev)
        wb = torch.empty_like(wa)

        def fused():
            Q.restoration_quality_hip(ref, [blurred, restored], out=out2, acc=acc, work=work2)

        def two():      # (no host-side fold counted for them)
            Q.psnr_ssim_hip(blurred, ref, out=oa, work=wa)
            Q.psnr_ssim_hip(restored, ref, out=ob, work=wb)

        def one():
            Q.psnr_ssim_hip(blurred, ref, out=oa, work=wa)
        arms = {"fused K=2 + acc": fused, "two psnr_ssim_hip": two, "one psnr_ssim_hip": one}
        for f in arms.values():
            timed(f, 5)
        res = {k: [] for k in arms}
        for _ in range(5):
            for k, f in arms.items():
                res[k] += timed(f)
        for k, ts in res.items():
            ts.sort()
            print("%s sharp Half, blurred Half, restored fp32  %-18s median %.1f us (%.1f .. %.1f)" % (shape, k, ts[len(ts) // 2], ts[0], ts[-1]),
                  flush=True)
        assert torch.equal(out2[:3].view(torch.int32), oa.view(torch.int32)) and torch.equal(out2[3:].view(torch.int32), ob.view(torch.int32))


def cell(n=200, passes=3, warm=8):
    from detectinblur_amd import evaluate as EV
    from detectinblur_amd import kernel_choices, train as TR, utils
    from detectinblur_amd.coco_utils import get_coco
    from detectinblur_amd.engine import evaluate
    from detectinblur_amd.models.deconvolve import Deconvolver
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    kernel_choices.use_shipped_kernel_choices()
    dev = torch.device("cuda:0")
    TR.seed_everything(False)
    model = fasterrcnn_resnet50_fpn(num_classes=91, pretrained=False, pretrained_backbone=False).to(dev).eval()
    kinds = (("deconvolve", {}), ("+ metrics", dict(restoration_metrics=True)))
    res, figures = {k: [] for k, _ in kinds}, None
    for rep in range(passes + 1):                                      # pass 0 of each kind warms up (on fewer images)
        for name, kw in kinds:
            count = n if rep else 16
            tf = TR.get_transform(False, blur=True, blur_type=EV.SWEEP_PARAMS[1], blur_ratio=1, blur_exposure=EV.SWEEP_FRACTIONS[2])
            dset, _ = get_coco(None, "val", tf, synthetic=dict(num_images=warm + count, size=(H, W)))
            loader = torch.utils.data.DataLoader(dset, batch_size=1, shuffle=False, num_workers=4, collate_fn=utils.collate_fn, pin_memory=True)
            stamps = []

            def stamped(it):
                for k, batch in enumerate(it):
                    if k == warm:
                        torch.cuda.synchronize()
                        stamps.append(time.perf_counter())
                    yield batch

            class L(object):
                dataset = dset

                def __iter__(self):
                    return stamped(iter(loader))

                def __len__(self):
                    return len(loader)
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                out = evaluate(model, L(), device=dev, blurring_images=True, gpu_blur=True, expand_target_boxes=True, deconvolve_first=True,
                               deconvolver=Deconvolver(N), **kw)
            torch.cuda.synchronize()
            ips = count / (time.perf_counter() - stamps[0])
            print("pass %d %-12s %6.2f images/s (%d timed images after %d; whole pass %.1f s)" % (rep, name, ips, count, warm, time.perf_counter() - t0),
                  flush=True)
            if rep:
                res[name].append(ips)
            if "restoration" in out:
                figures = out["restoration"]
    for name, _ in kinds:
        v = res[name]
        print("sweep cell P2 E3 at %d x %d, %-12s median %6.2f images/s (%s) = %.2f ms per image" % (H, W, name, np.median(v),
                                                                                                ", ".join("%.2f" % x for x in v), 1000 / np.median(v)))
    from detectinblur_amd.quality import format_restoration
    print(format_restoration(figures))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "call":
        call()
    elif mode == "cell":
        cell(int(sys.argv[2]) if len(sys.argv) > 2 else 200)
    else:
        raise SystemExit(__doc__)
