"""--deconvolve_tv on one MI355X: what profiles/deconvolve_tv.txt records.

    python scratch/deconvolve_tv_timing.py kernel         dib_tv_weight per 3 x 800 x 1333 plane set (fp32 and Half input) against the torch
                                                          restatement on the same GPU, alternated; graph replays of 48 launches that cycle
                                                          through 12 input / output pairs (more than the 256 MiB the last-level cache holds)
    python scratch/deconvolve_tv_timing.py trace          the same launches, eager, for `rocprofv3 --kernel-trace --stats -- python ... trace`
    python scratch/deconvolve_tv_timing.py stage          the N = 30 stage with and without tv_lambda = 0.01 for the two PSFs of
                                                          profiles/deconvolve_first.txt (12 and 247 taps), alternated
    python scratch/deconvolve_tv_timing.py cell [IMAGES]  sweep cell P2 E3 at 800 x 1333 under --add_noise with --restoration_metrics:
                                                          --deconvolve_first without and with --deconvolve_tv 0.01, alternated three times
"""
import contextlib
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scratch.deconvolve_timing import _event_ms, sweep_psf      # noqa: E402

C, H, W, N = 3, 800, 1333, 30
LAMBDA, BETA = 0.01, 1e-2
PAIRS, LAUNCHES = 12, 48


def _summary(v):
    return "%.2f us (min %.2f, max %.2f)" % (np.median(v), min(v), max(v))


def _planes(dtype, dev):
    g = torch.Generator().manual_seed(0)
    return [torch.rand(C, H, W, generator=g).to(dtype).to(dev) for _ in range(PAIRS)]


def kernel(rounds=10):
    from detectinblur_amd import _lib
    from detectinblur_amd.models import deconvolve as DC
    dev = torch.device("cuda:0")
    l = _lib.lib()
    arms, graphs = {}, {}
    outs = [torch.empty(C, H, W, dtype=torch.float32, device=dev) for _ in range(PAIRS)]
    for name, dtype, code in (("fp32", torch.float32, _lib.DIB_F32), ("half", torch.float16, _lib.DIB_F16)):
        xs = _planes(dtype, dev)

        def hip(xs=xs, code=code):
            s = _lib.stream_of(xs[0])
            for k in range(LAUNCHES):
                _lib.check(l.dib_tv_weight(xs[k % PAIRS].data_ptr(), code, outs[k % PAIRS].data_ptr(), C, H, W, LAMBDA, BETA, s))
        arms["hip " + name] = hip
        if dtype == torch.float32:
            arms["torch fp32"] = lambda xs=xs: [DC.tv_weight_torch(xs[k % PAIRS], LAMBDA, BETA) for k in range(PAIRS)]
            err = float((DC.tv_weight(xs[0], LAMBDA, BETA) - DC.tv_weight_torch(xs[0], LAMBDA, BETA)).abs().max())
    for name, fn in arms.items():
        fn()
        torch.cuda.synchronize()
        if name.startswith("hip"):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fn()
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn()
            graphs[name] = g
    per = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            if name in graphs:
                graphs[name].replay()      # once untimed: the replay's own start-up is not the kernel's
                per[name].append(1e3 * _event_ms(graphs[name].replay) / LAUNCHES)
            else:
                per[name].append(1e3 * _event_ms(fn) / PAIRS)
    px = C * H * W
    for name, v in per.items():
        line = "%-10s per 3 x %d x %d plane set: %s over %d rounds" % (name, H, W, _summary(v), rounds)
        if name.startswith("hip"):
            nbytes = px * (8 if name.endswith("fp32") else 6)
            line += " | %.1f MB algorithmic = %.2f TB/s; the 8 TB/s floor is %.2f us: %.0f %% of it" % (
                nbytes / 1e6, nbytes / np.median(v) / 1e6, nbytes / 8e6, 100 * (nbytes / 8e6) / np.median(v))
        print(line, flush=True)
    print("torch / hip (fp32): %.1f | HIP against torch on one plane set: %.2e" % (np.median(per["torch fp32"]) / np.median(per["hip fp32"]), err))
    print("(graph replays of %d launches over %d buffer pairs: a launch's figure includes the boundary to the next kernel)" % (LAUNCHES, PAIRS))


def trace():
    from detectinblur_amd import _lib
    dev = torch.device("cuda:0")
    l = _lib.lib()
    outs = [torch.empty(C, H, W, dtype=torch.float32, device=dev) for _ in range(PAIRS)]
    for dtype, code in ((torch.float32, _lib.DIB_F32), (torch.float16, _lib.DIB_F16)):
        xs = _planes(dtype, dev)
        for k in range(4 * LAUNCHES):
            _lib.check(l.dib_tv_weight(xs[k % PAIRS].data_ptr(), code, outs[k % PAIRS].data_ptr(), C, H, W, LAMBDA, BETA, _lib.stream_of(xs[0])))
        torch.cuda.synchronize()


def stage(reps=7):
    from detectinblur_amd import blur_ops
    from detectinblur_amd.models import deconvolve as DC
    dev = torch.device("cuda:0")
    sharp = torch.rand(3, H, W, generator=torch.Generator().manual_seed(0)).half().to(dev)
    for label, fraction in (("E = 1/25", 1 / 25), ("E = 1", 1.0)):
        psf = sweep_psf(0.001, fraction, seed=1337).to(dev)
        tables = blur_ops.compact_psfs([psf], normalize=True)
        y = blur_ops.sparse_blur([sharp], [0], tables)[0]
        plain = lambda: DC.richardson_lucy_hip(y, tables, 0, N)                                # noqa: E731
        tv = lambda: DC.richardson_lucy_hip(y, tables, 0, N, 1e-6, LAMBDA, BETA)               # noqa: E731
        for fn in (plain, tv):
            fn()
        torch.cuda.synchronize()
        t_plain, t_tv = [], []
        for _ in range(reps):
            t_plain.append(_event_ms(plain))
            t_tv.append(_event_ms(tv))
        m_plain, m_tv = np.median(t_plain), np.median(t_tv)
        print("%-8s %4d taps: plain %.3f ms (min %.3f, max %.3f) | tv_lambda %g: %.3f ms (min %.3f, max %.3f) | %d runs each, alternated | "
              "+%.3f ms = +%.1f us per iteration = x %.3f" % (label, tables.header(0)[0], m_plain, min(t_plain), max(t_plain), LAMBDA, m_tv, min(t_tv),
                                                           max(t_tv), reps, m_tv - m_plain, 1e3 * (m_tv - m_plain) / N, m_tv / m_plain), flush=True)


def cell(n=200, passes=3, warm=8):
    from detectinblur_amd import evaluate as EV
    from detectinblur_amd import kernel_choices, train as TR, utils
    from detectinblur_amd.coco_utils import get_coco
    from detectinblur_amd.engine import evaluate
    from detectinblur_amd.models.deconvolve import Deconvolver
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    from detectinblur_amd.quality import format_restoration
    kernel_choices.use_shipped_kernel_choices()
    dev = torch.device("cuda:0")
    TR.seed_everything(False)
    model = fasterrcnn_resnet50_fpn(num_classes=91, pretrained=False, pretrained_backbone=False).to(dev).eval()
    kinds = (("plain", Deconvolver(N)), ("tv %g" % LAMBDA, Deconvolver(N, tv_lambda=LAMBDA, tv_beta=BETA)))
    res, figures = {k: [] for k, _ in kinds}, {}
    for rep in range(passes + 1):                                      # pass 0 of each kind warms up (on fewer images)
        for name, deconvolver in kinds:
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
                               deconvolver=deconvolver, add_noise=True, restoration_metrics=True)
            torch.cuda.synchronize()
            ips = count / (time.perf_counter() - stamps[0])
            print("pass %d %-8s %6.2f images/s (%d timed images after %d; whole pass %.1f s)" % (rep, name, ips, count, warm, time.perf_counter() - t0),
                  flush=True)
            if rep:
                res[name].append(ips)
                figures[name] = out["restoration"]
    for name, _ in kinds:
        v = res[name]
        print("sweep cell P2 E3 at %d x %d under --add_noise, %-8s median %6.2f images/s (%s) = %.2f ms per image" % (
            H, W, name, np.median(v), ", ".join("%.2f" % x for x in v), 1000 / np.median(v)))
        print("    %s" % format_restoration(figures[name]))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode in ("kernel", "trace", "stage"):
        {"kernel": kernel, "trace": trace, "stage": stage}[mode]()
    elif mode == "cell":
        cell(int(sys.argv[2]) if len(sys.argv) > 2 else 200)
    else:
        raise SystemExit(__doc__)
