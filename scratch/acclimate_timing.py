"""--acclimate_norm against --mode_one_norm and frozen batch-norm (profiles/acclimate_norm.txt).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/<run> -o t -- python scratch/acclimate_timing.py trace mode_one|acclimate
    python scratch/acclimate_timing.py report OUT/<run> [OUT/<run> ...]
    python scratch/acclimate_timing.py cell [images] [workers]

`trace`: the converted detector's trunk (53 batch-norm layers behind their convolutions) on 10 synthetic 800 x 1344 images, eager,
batch 1; all of them are in the trace, and the report divides by the launches it counts.
`report`: per run, the device time of the three batch-norm launches per image (one image = 53 partial-statistics launches), summed
from the trace's statistics file.
`cell`: engine.evaluate as the sweep calls it (P1E1, --gpu_blur --expand_target_boxes, random init, synthetic 800 x 1333 images through
the loader, graphed trunk), `images` timed images after 8: frozen batch-norm, --mode_one_norm and --acclimate_norm (cumulative
average, prior 16), alternated three times.
"""
import contextlib
import csv
import glob
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from detectinblur_amd import utils  # noqa: E402
from detectinblur_amd.models.batchnorm import BatchNorm2d  # noqa: E402

KERNELS = (("partial", "bn_partial_kernel"), ("finalize", "bn_finalize_kernel"), ("finalize", "bn_acclimate_finalize_kernel"),
           ("apply", "bn_apply_kernel"), ("apply", "bn_apply_bump_kernel"))


def _model(mode, dev):
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    torch.manual_seed(0)
    m = fasterrcnn_resnet50_fpn(num_classes=91, pretrained=False, pretrained_backbone=False).to(dev).eval()
    if mode == "frozen":
        return m
    m = utils.set_batch_norm_N(utils.convert_to_custom_batch_norm(m, batch_norm_to_use=BatchNorm2d), 16)
    if mode == "mode_one":
        return utils.set_batch_norm_mode1(m, True).eval()
    m = utils.set_batch_norm_acclimation_mode(utils.set_batch_momentum_zero(m), True)
    m = utils.copy_BN_stats_to_old(m).eval()
    m.acclimate_norm, m.acclimation_carry_over = True, False
    return utils.turn_batch_norm_on(m)


def trace(mode):
    from detectinblur_amd import kernel_choices
    kernel_choices.use_shipped_kernel_choices()
    dev = torch.device("cuda:0")
    m = _model(mode, dev)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for _ in range(10):
            x = torch.rand((1, 3, 800, 1344), generator=g).to(dev).contiguous(memory_format=torch.channels_last)
            m.backbone(x)
    torch.cuda.synchronize()
    paths = {b.last_path for b in m.modules() if isinstance(b, BatchNorm2d)}
    assert paths == {"hip"}, paths


def report(dirs):
    totals = []
    for d in dirs:
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        assert len(files) == 1, (d, files)
        t, calls = {"partial": 0.0, "finalize": 0.0, "apply": 0.0}, 0
        for r in csv.DictReader(open(files[0])):
            for what, frag in KERNELS:
                if ("dib::" + frag + "(") in r["Name"] or ("dib::" + frag + "<") in r["Name"]:
                    t[what] += float(r["TotalDurationNs"])
                    calls += int(r["Calls"]) if what == "partial" else 0
        images = calls / 53.0
        per = {k: v / images / 1e3 for k, v in t.items()}
        totals.append(sum(per.values()))
        print("%-28s images %4.1f: partial %6.1f us, finalize %6.1f us, apply %6.1f us, total %7.1f us per image"
              % (os.path.basename(d.rstrip("/")), images, per["partial"], per["finalize"], per["apply"], totals[-1]))
    return totals


class _Timed(object):
    """A loader that stamps the clock in front of batch `warm`."""

    def __init__(self, loader, warm):
        self.loader, self.warm, self.stamps, self.dataset = loader, warm, [], loader.dataset

    def __iter__(self):
        for k, batch in enumerate(iter(self.loader)):
            if k == self.warm:
                torch.cuda.synchronize()
                self.stamps.append(time.perf_counter())
            yield batch

    def __len__(self):
        return len(self.loader)


def cell(n=200, workers=8):
    from detectinblur_amd import evaluate as EV
    from detectinblur_amd import kernel_choices
    from detectinblur_amd import train as TR
    from detectinblur_amd.coco_utils import get_coco
    from detectinblur_amd.engine import evaluate
    ctx = utils.loader_context() if workers else None
    kernel_choices.use_shipped_kernel_choices()
    TR.seed_everything(False)
    dev = torch.device("cuda:0")
    modes = ("frozen", "mode_one", "acclimate")
    models = {mode: _model(mode, dev) for mode in modes}
    warm = 8
    rates = {mode: [] for mode in modes}
    for rep in range(-1, 3):                                          # rep -1: a short untimed pass (graph capture, kernel choices)
        for mode in modes:
            count = warm + (n if rep >= 0 else 8)
            with contextlib.redirect_stdout(io.StringIO()):
                tf = TR.get_transform(False, blur=True, blur_type=EV.SWEEP_PARAMS[0], blur_ratio=1, blur_exposure=EV.SWEEP_FRACTIONS[0])
                ds, _ = get_coco(None, "val", tf, synthetic=dict(num_images=count, size=(800, 1333)))
            loader = _Timed(torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, num_workers=workers, collate_fn=utils.collate_fn,
                                                        pin_memory=True, multiprocessing_context=ctx), warm)
            with contextlib.redirect_stdout(io.StringIO()):
                evaluate(models[mode], loader, device=dev, blurring_images=True, gpu_blur=True, expand_target_boxes=True)
            torch.cuda.synchronize()
            took = time.perf_counter() - loader.stamps[0]
            if rep < 0:
                continue
            rates[mode].append(n / took)
            extra = ""
            if mode == "acclimate":
                counters = {int(b.num_batches_tracked) for b in models[mode].modules() if isinstance(b, BatchNorm2d)}
                graphs = models[mode].__dict__.get("_trunk_graphs")
                extra = "  counters %s, trunk graphs %d" % (sorted(counters), 0 if graphs is None else sum(v is not None for v in graphs.graphs.values()))
            print("rep %d  %-9s %6.1f images/s  (%d images after %d)%s" % (rep, mode, n / took, n, warm, extra), flush=True)
    for mode in modes:
        print("median %-9s %6.1f images/s  runs %s" % (mode, float(np.median(rates[mode])), ", ".join("%.1f" % r for r in rates[mode])))


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "trace":
        trace(sys.argv[2])
    elif what == "report":
        report(sys.argv[2:])
    elif what == "cell":
        cell(*[int(a) for a in sys.argv[2:4]])
    else:
        raise SystemExit(__doc__)
