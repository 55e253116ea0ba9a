"""The fused squint warp (csrc/dib_warp.hip) on one MI355X: what profiles/squint_warp.txt records.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/fused -o t -- python scratch/squint_warp_timing.py kernels fused
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/torch -o t -- python scratch/squint_warp_timing.py kernels torch
    python scratch/squint_warp_timing.py report OUT/fused OUT/torch    device time and launches per warp from the two traces
    python scratch/squint_warp_timing.py train [steps]    loader-fed b = 8 train step with --warp_in_model, fused and torch path alternated, 3 reps
    python scratch/squint_warp_timing.py cell             sweep cell P1E1 at batch 1 with --warp_in_model: graphed fused trunk against the
                                                          plain loop with the torch path (DIB_NO_FUSED_WARP=1: what the code did before)

`kernels`: the six warps of one b = 8 step at 800 x 1344 (the image, then the five FPN levels at 256 channels with the inverse
scales), channels-last float32.  Per shape a section of REPS forward calls and (levels only) a section of REPS backward calls,
each between two marker kernels (torch.cuda._sleep: `spin_kernel`) which `report` finds in the trace again.  The torch path is Warper(): the op chain the fused
kernels replace."""
import csv
import glob
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, H, W = 8, 800, 1333
SHAPES = [(8, 3, 800, 1344), (8, 256, 200, 336), (8, 256, 100, 168), (8, 256, 50, 84), (8, 256, 25, 42), (8, 256, 13, 21)]
REPS = 5


def kernels(mode):
    from detectinblur_amd.models.warper import Warper
    dev = torch.device("cuda:0")
    w = Warper(fused=(mode == "fused"))
    g = torch.Generator().manual_seed(0)
    th = (torch.rand(B, generator=g) * 3 - 1.5).half().to(dev)
    l1 = (0.7 + 0.3 * torch.rand(B, generator=g)).half().to(dev)
    l2 = (0.7 + 0.3 * torch.rand(B, generator=g)).half().to(dev)
    for shape in SHAPES:
        level = shape[1] != 3
        x = torch.randn(shape, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(level)
        go = torch.randn(shape, device=dev).contiguous(memory_format=torch.channels_last)
        a, b = (1 / l1, 1 / l2) if level else (l1, l2)
        for timed in (False, True):          # a warm-up round of the timed round's shape: allocations, code loading, table upload
            mark = torch.cuda._sleep if timed else (lambda cycles: None)
            mark(1000)
            outs = [w(x, th, a, b) for _ in range(REPS)]
            mark(1000)
            torch.cuda.synchronize()
            if level:
                mark(1000)
                for o in outs:
                    torch.autograd.grad(o, x, go)
                mark(1000)
            torch.cuda.synchronize()
            del outs
        del x, go
    print("%s: done" % mode)


def _sections(d):
    path = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[0]
    with open(path) as f:
        rows = list(csv.DictReader(f))
    kn = "Kernel_Name" if "Kernel_Name" in rows[0] else "Name"
    ev = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r[kn]) for r in rows), key=lambda e: e[0])
    out, cur = [], None                   # the kernels between marker 2k and marker 2k + 1
    for a, b, n in ev:
        if "spin_kernel" in n:
            if cur is None:
                cur = []
            else:
                out.append(cur)
                cur = None
        elif cur is not None:
            cur.append((a, b, n))
    assert cur is None
    return out


def report(dirs):
    """Per shape: [forward x REPS, (backward x REPS)] sections in trace order."""
    print("shape | pass | path: device us per call, launches per call (matrix computation included: squint_matrices is the same on both paths)")
    per = {}
    for d, name in zip(dirs, ("fused", "torch")):
        secs = _sections(d)
        k = 0
        for shape in SHAPES:
            level = shape[1] != 3
            for what in (("forward", "backward") if level else ("forward",)):
                s = secs[k]
                k += 1
                warp = [e for e in s if "squint" in e[2]]
                if name == "fused":          # the sections are the ones that were marked: REPS kernels of the right pass, nothing else of ours
                    assert len(warp) == REPS and all(("squint_bwd" in e[2]) == (what == "backward") for e in warp), (shape, what, len(s), [e[2][:40] for e in warp])
                per[(shape, what, name)] = (sum(b - a for a, b, _ in s) / 1e3 / REPS, len(s) / REPS, sum(b - a for a, b, _ in warp) / 1e3 / REPS, len(warp) / REPS)
    for shape in SHAPES:
        for what in ("forward", "backward"):
            if (shape, what, "fused") not in per:
                continue
            f, t = per[(shape, what, "fused")], per[(shape, what, "torch")]
            elems = float(np.prod(shape))
            print("%-20s %-8s fused %8.1f us, %5.1f launches (the dib kernel alone: %8.1f us, %.2f TB/s at %d B per element%s) | torch %8.1f us, %5.1f launches" % (
                shape, what, f[0], f[1], f[2], elems * (8 if what == "forward" else 16) / (f[2] * 1e-6) / 1e12 if f[2] else 0.0,
                8 if what == "forward" else 16, "" if what == "forward" else " added by atomics", t[0], t[1]))
    for name in ("fused", "torch"):
        tot = {w_: sum(v[0] for k_, v in per.items() if k_[1] == w_ and k_[2] == name) for w_ in ("forward", "backward")}
        n = {w_: sum(v[1] for k_, v in per.items() if k_[1] == w_ and k_[2] == name) for w_ in ("forward", "backward")}
        print("%s, all six warps of a b = 8 step: forward %.2f ms in %.0f launches, backward (five levels) %.2f ms in %.0f launches" % (
            name, tot["forward"] / 1e3, n["forward"], tot["backward"] / 1e3, n["backward"]))


def _model(dev):
    from detectinblur_amd import kernel_choices
    from detectinblur_amd import train as TR
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    kernel_choices.use_shipped_kernel_choices()
    TR.seed_everything(False)
    return fasterrcnn_resnet50_fpn(num_classes=91, pretrained=False, pretrained_backbone=False, warp_internally=True).to(dev)


class _Timed(object):
    """A loader that stamps the clock in front of batch `warm`."""

    def __init__(self, loader, warm, dataset=None):
        self.loader, self.warm, self.stamps, self.dataset = loader, warm, [], dataset

    def __iter__(self):
        for k, batch in enumerate(iter(self.loader)):
            if k == self.warm:
                torch.cuda.synchronize()
                self.stamps.append(time.perf_counter())
            yield batch

    def __len__(self):
        return len(self.loader)


def _set_path(name):
    if name == "fused":
        os.environ.pop("DIB_NO_FUSED_WARP", None)
    else:
        os.environ["DIB_NO_FUSED_WARP"] = "1"


def train(steps):
    from detectinblur_amd import train as TR
    from detectinblur_amd import utils
    from detectinblur_amd.coco_utils import get_coco
    from detectinblur_amd.engine import train_one_epoch
    dev = torch.device("cuda:0")
    model = _model(dev)
    opt = utils.make_sgd([p for p in model.parameters() if p.requires_grad], 0.0001, 0.9, 1e-4)
    warm = 5
    results = {"torch path": [], "fused": []}
    for rep in range(3):
        for name in results:
            _set_path(name)
            tf = TR.get_transform(True, blur=True, blur_ratio=0.9)
            ds, _ = get_coco(None, "train", tf, synthetic=dict(num_images=(warm + steps) * B, size=(H, W)))
            loader = _Timed(torch.utils.data.DataLoader(ds, batch_size=B, shuffle=False, num_workers=8, collate_fn=utils.collate_fn, pin_memory=True,
                                                        worker_init_fn=TR._seed_worker, persistent_workers=False, prefetch_factor=4), warm)
            train_one_epoch(model, opt, loader, dev, epoch=1, print_freq=10 ** 6, blur_train=True, early_stop=None, gpu_blur=True,
                            expand_target_boxes=True)
            torch.cuda.synchronize()
            ips = steps * B / (time.perf_counter() - loader.stamps[0])
            results[name].append(ips)
            print("rep %d  %-10s %6.1f images/s  (%.1f ms per step)" % (rep, name, ips, 1000 * B / ips), flush=True)
    base = np.median(results["torch path"])
    for name, v in results.items():
        print("median %-10s %6.1f images/s  (%+.1f %% vs torch path)  runs %s" % (name, np.median(v), 100 * (np.median(v) / base - 1),
                                                                                ", ".join("%.1f" % x for x in v)))


def cell():
    import contextlib
    import io
    from detectinblur_amd import evaluate as EV
    from detectinblur_amd import train as TR
    from detectinblur_amd import utils
    from detectinblur_amd.coco_utils import get_coco
    from detectinblur_amd.engine import evaluate
    dev = torch.device("cuda:0")
    model = _model(dev).eval()
    warm, n = 4, 16
    out = []
    for name in ("torch path, plain loop", "fused, graphed trunk", "torch path, plain loop again"):
        _set_path("fused" if name.startswith("fused") else "torch")
        tf = TR.get_transform(False, blur=True, blur_type=EV.SWEEP_PARAMS[0], blur_ratio=1, blur_exposure=EV.SWEEP_FRACTIONS[0])
        ds, _ = get_coco(None, "val", tf, synthetic=dict(num_images=warm + n, size=(H, W)))
        loader = _Timed(torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, num_workers=0, collate_fn=utils.collate_fn, pin_memory=True), warm, ds)
        with contextlib.redirect_stdout(io.StringIO()):
            evaluate(model, loader, device=dev, blurring_images=True, gpu_blur=True, expand_target_boxes=True)
        torch.cuda.synchronize()
        out.append("%s %.1f" % (name, n / (time.perf_counter() - loader.stamps[0])))
        cache = model.__dict__.get("_warped_trunk_graphs")
        if name.startswith("fused"):
            out[-1] += " (%d captured shapes)" % (0 if cache is None else sum(g is not None for g in cache.graphs.values()))
    print("sweep cell P1E1 with --warp_in_model, %d timed images after %d, images/s (COCO accumulation of the cell included): %s" % (n, warm, " | ".join(out)))


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "kernels":
        kernels(sys.argv[2])
    elif mode == "report":
        report(sys.argv[2:4])
    elif mode == "train":
        train(int(sys.argv[2]) if len(sys.argv) > 2 else 30)
    elif mode == "cell":
        cell()
    else:
        raise SystemExit(__doc__)
