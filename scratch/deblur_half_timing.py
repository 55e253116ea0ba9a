"""--deblur_precision half on one MI355X: what profiles/deblur_half.txt records.

    python scratch/deblur_half_timing.py stage              the whole stage per image at 480 x 640 and 800 x 1333, single and half alternated
    python scratch/deblur_half_timing.py cell               sweep cell P2 E3 at 800 x 1333: without the stage, single, half, alternated
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o t -- python scratch/deblur_half_timing.py steps
    python scratch/deblur_half_timing.py report OUT         device time per kernel from that trace: the project's kernels in both forms,
                                                            the convolutions' share and rate in both precisions, MIOpen's kernel names

The deblurrer is write_random_checkpoint at the default architecture (n_scales 3, n_resblocks 19, n_feats 64, k 5; seed 0): device time does
not depend on the values.  Nothing is tuned and no find-db record exists for these convolutions in either precision: the first calls of
every shape hold MIOpen's searches, and their wall time is printed."""
import contextlib
import csv
import glob
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = ((480, 640), (800, 1333))
PRECISIONS = ("single", "half")


def conv_flop(h, w, n_scales=3, n_resblocks=19, n_feats=64, k=5):
    """multiply-adds x 2 of every convolution of one pass, from the shapes (padded to a multiple of 2 ** (n_scales - 1))"""
    d = 1 << (n_scales - 1)
    hp, wp = -(-h // d) * d, -(-w // d) * d
    total = 0
    for s in range(n_scales):
        px = (hp >> s) * (wp >> s)
        cin = 6 if s < n_scales - 1 else 3
        per_px = cin * n_feats + 2 * n_resblocks * n_feats * n_feats + n_feats * 3 + (3 * 12 if s > 0 else 0)
        total += 2 * k * k * per_px * px
    return total


def _deblurrers(dev):
    from detectinblur_amd import kernel_choices
    from detectinblur_amd.models.deblur import Deblurer, write_random_checkpoint
    kernel_choices.use_shipped_kernel_choices()
    d = tempfile.mkdtemp(prefix="dib_deblur_timing_")
    write_random_checkpoint(d, seed=0)
    with contextlib.redirect_stdout(io.StringIO()):
        return {p: Deblurer(d, dev, precision=p) for p in PRECISIONS}


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stage(reps=7):
    dev = torch.device("cuda:0")
    ds = _deblurrers(dev)
    g = torch.Generator().manual_seed(0)
    for h, w in SIZES:
        x = torch.rand(3, h, w, generator=g).half().to(dev)
        for p in PRECISIONS:                                           # the first calls: MIOpen's searches
            t0 = time.perf_counter()
            for _ in range(2):
                ds[p].deblur_(x)
            torch.cuda.synchronize()
            assert ds[p].last_path == "hip"
            print("%d x %d %-6s first two calls (MIOpen searches every new shape): %.1f s" % (h, w, p, time.perf_counter() - t0), flush=True)
        runs = {p: [] for p in PRECISIONS}
        for _ in range(reps):
            for p in PRECISIONS:
                runs[p].append(_event_ms(lambda: ds[p].deblur_(x)))
        # the project's own launches alone: the stage with every convolution replaced by an empty tensor of its shape would change the
        # graph; instead `report` reads them from the trace.  Here: the stage, and the difference between the precisions.
        out = ds["half"].deblur_(x).float()
        ref = ds["single"].deblur_(x)
        flop = conv_flop(h, w)
        for p in PRECISIONS:
            v = np.array(runs[p])
            print("%d x %d %-6s stage per image: median %.2f ms (min %.2f, max %.2f, %d alternated runs); %.2f TFLOP of convolutions -> %.0f TFLOP/s "
                  "over the whole stage" % (h, w, p, np.median(v), v.min(), v.max(), reps, flop / 1e12, flop / (np.median(v) * 1e-3) / 1e12), flush=True)
        print("%d x %d half against single: %.2fx; largest difference of the outputs (scale 0..1) %.2e" % (
            h, w, np.median(runs["single"]) / np.median(runs["half"]), float((out - ref).abs().max())), flush=True)


def cell(passes=3):
    from detectinblur_amd import evaluate as EV
    from detectinblur_amd import train as TR
    from detectinblur_amd import utils
    from detectinblur_amd.coco_utils import get_coco
    from detectinblur_amd.engine import evaluate
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    dev = torch.device("cuda:0")
    ds = _deblurrers(dev)
    TR.seed_everything(False)
    model = fasterrcnn_resnet50_fpn(num_classes=91, pretrained=False, pretrained_backbone=False).to(dev).eval()
    h, w = SIZES[1]
    warm, n = 4, 16
    kinds = (("without", None), ("single", ds["single"]), ("half", ds["half"]))
    res = {k: [] for k, _ in kinds}
    for rep in range(passes + 1):                                      # pass 0 of each kind warms up
        for name, d in kinds:
            tf = TR.get_transform(False, blur=True, blur_type=EV.SWEEP_PARAMS[1], blur_ratio=1, blur_exposure=EV.SWEEP_FRACTIONS[2])
            dset, _ = get_coco(None, "val", tf, synthetic=dict(num_images=warm + n, size=(h, w)))
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
                evaluate(model, L(), device=dev, blurring_images=True, gpu_blur=True, expand_target_boxes=True, deblur_first=d is not None, deblurer=d)
            torch.cuda.synchronize()
            ips = n / (time.perf_counter() - stamps[0])
            print("pass %d %-8s %6.2f images/s (%d timed images after %d; whole pass %.1f s)" % (rep, name, ips, n, warm, time.perf_counter() - t0), flush=True)
            if rep:
                res[name].append(ips)
    for name, _ in kinds:
        v = res[name]
        print("sweep cell P2 E3 at %d x %d, %-8s median %6.2f images/s (%s) = %.1f ms per image" % (h, w, name, np.median(v), ", ".join("%.2f" % x for x in v),
                                                                                             1000 / np.median(v)))


def steps(n=3):
    """under the tracer: warm-up (searches), a gap, then n images per precision at 800 x 1333, single first; a gap between the two"""
    dev = torch.device("cuda:0")
    ds = _deblurrers(dev)
    h, w = SIZES[1]
    x = torch.rand(3, h, w, generator=torch.Generator().manual_seed(0)).half().to(dev)
    for p in PRECISIONS:
        for _ in range(2):
            ds[p].deblur_(x)
    torch.cuda.synchronize()
    for p in PRECISIONS:
        time.sleep(1.0)
        for _ in range(n):
            ds[p].deblur_(x)
        torch.cuda.synchronize()
    print("traced %d images per precision at %d x %d" % (n, h, w))


def report(d, n=3):
    path = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[0]
    with open(path) as f:
        rows = list(csv.DictReader(f))
    kn = "Kernel_Name" if "Kernel_Name" in rows[0] else "Name"
    ev = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r[kn]) for r in rows), key=lambda e: e[0])
    cuts, last_end = [], ev[0][1]
    for i, (a, b, _) in enumerate(ev):
        if a - last_end >= 0.5e9:
            cuts.append(i)
        last_end = max(last_end, b)
    assert len(cuts) >= 2, "expected the two gaps `steps` sleeps through"
    windows = {"single": ev[cuts[-2]:cuts[-1]], "half": ev[cuts[-1]:]}
    h, w = SIZES[1]
    flop = conv_flop(h, w)
    for p, win in windows.items():
        per = {}
        for a, b, name in win:
            t, c = per.get(name, (0.0, 0))
            per[name] = (t + (b - a) / 1e3, c + 1)
        own = {k: v for k, v in per.items() if "dib::" in k}
        other = {k: v for k, v in per.items() if "dib::" not in k}
        t_own, t_other = sum(t for t, _ in own.values()) / n, sum(t for t, _ in other.values()) / n
        print("%s: device time per image %.2f ms in %d kernels; the project's kernels %.3f ms (%.2f %%), everything else (MIOpen's convolutions and "
              "what torch runs around them) %.2f ms -> %.0f TFLOP/s over %.2f TFLOP" % (p, (t_own + t_other) / 1e3, len(win) // n, t_own / 1e3,
                                                                                       100 * t_own / (t_own + t_other), t_other / 1e3,
                                                                                       flop / (t_other * 1e-6) / 1e12, flop / 1e12))
        print("  the project's kernels (us per call, calls per image, us per image, name):")
        for k, (t, c) in sorted(own.items(), key=lambda kv: kv[0]):
            print("    %8.2f %6.1f %9.1f  %s" % (t / c, c / n, t / n, k[:150]))
        print("  everything else (us per call, calls per image, ms per image, name):")
        for k, (t, c) in sorted(other.items(), key=lambda kv: -kv[1][0])[:8]:
            print("    %8.1f %6.1f %9.2f  %s" % (t / c, c / n, t / n / 1e3, k[:150]))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "stage":
        stage()
    elif mode == "cell":
        cell()
    elif mode == "steps":
        steps()
    elif mode == "report":
        report(sys.argv[2])
    else:
        raise SystemExit(__doc__)
