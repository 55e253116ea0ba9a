"""--amp (bf16 trunk) on one MI355X: what profiles/amp_trunk.txt records.

    python scratch/amp_timing.py train [steps]          loader-fed b = 8 train step, fp32 and --amp alternated, 3 reps each
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/fp32 -o t -- python scratch/amp_timing.py steps fp32
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/amp -o t -- python scratch/amp_timing.py steps amp
    python scratch/amp_timing.py report OUT/fp32 OUT/amp      device time per kernel family from the two traces
    python scratch/amp_timing.py cell                    sweep cell P1E1, single detector, graphed trunk, fp32 / --amp / fp32
    python scratch/amp_timing.py convs                   per bf16 convolution of the b = 1 trunk: run-to-run identity and time of
                                                         MIOpen's channels-last kernel against the GEMM (1x1) / planar (3x3) detour

`train`: engine.train_one_epoch on fasterrcnn_resnet50_fpn (random init: all five stages train), synthetic 3 x 800 x 1333 through
the loader (8 workers), --blur_train --gpu_blur --expand_target_boxes, as profiles/augmix.txt ran it.  `steps`: 5 + 10 train steps
on one device-resident batch (no loader, no blur), the ten under the trace."""
import csv
import glob
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, H, W = 8, 800, 1333
BF = torch.bfloat16


def _model(dev):
    from detectinblur_amd import kernel_choices
    from detectinblur_amd import train as TR
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    kernel_choices.use_shipped_kernel_choices()
    TR.seed_everything(False)
    return fasterrcnn_resnet50_fpn(num_classes=91, pretrained=False, pretrained_backbone=False).to(dev)


def train(steps):
    from detectinblur_amd import train as TR
    from detectinblur_amd import utils
    from detectinblur_amd.coco_utils import get_coco
    from detectinblur_amd.engine import train_one_epoch
    dev = torch.device("cuda:0")
    model = _model(dev)
    opt = utils.make_sgd([p for p in model.parameters() if p.requires_grad], 0.0001, 0.9, 1e-4)
    warm = 5
    configs = {"fp32": torch.float32, "--amp": BF}
    results = {k: [] for k in configs}
    for rep in range(3):
        for name, dt in configs.items():
            model.backbone.compute_dtype = dt
            tf = TR.get_transform(True, blur=True, blur_ratio=0.9)
            ds, _ = get_coco(None, "train", tf, synthetic=dict(num_images=(warm + steps) * B, size=(H, W)))
            loader = torch.utils.data.DataLoader(ds, batch_size=B, shuffle=False, num_workers=8, collate_fn=utils.collate_fn, pin_memory=True,
                                                 worker_init_fn=TR._seed_worker, persistent_workers=False, prefetch_factor=4)
            stamps = []

            def timed(it):
                for k, batch in enumerate(it):
                    if k == warm:
                        torch.cuda.synchronize()
                        stamps.append(time.perf_counter())
                    yield batch

            class L(object):
                def __iter__(self):
                    return timed(iter(loader))

                def __len__(self):
                    return len(loader)
            train_one_epoch(model, opt, L(), dev, epoch=1, print_freq=10 ** 6, blur_train=True, early_stop=None, gpu_blur=True,
                            expand_target_boxes=True)
            torch.cuda.synchronize()
            ips = steps * B / (time.perf_counter() - stamps[0])
            results[name].append(ips)
            print("rep %d  %-8s %6.1f images/s  (%.1f ms per step)" % (rep, name, ips, 1000 * B / ips), flush=True)
    base = np.median(results["fp32"])
    for name, v in results.items():
        print("median %-8s %6.1f images/s  (%+.1f %% vs fp32)  runs %s" % (name, np.median(v), 100 * (np.median(v) / base - 1),
                                                                          ", ".join("%.1f" % x for x in v)))


def steps(mode):
    from detectinblur_amd import utils
    dev = torch.device("cuda:0")
    model = _model(dev).train()
    model.backbone.compute_dtype = BF if mode == "amp" else torch.float32
    opt = utils.make_sgd([p for p in model.parameters() if p.requires_grad], 0.0001, 0.9, 1e-4)
    g = torch.Generator().manual_seed(0)
    imgs = [torch.rand(3, H, W, generator=g).to(dev) for _ in range(B)]
    tg = [{"boxes": torch.tensor([[30., 40., 400., 460.], [100., 20., 700., 580.]], device=dev), "labels": torch.tensor([3, 17], device=dev)} for _ in range(B)]
    means, stds = np.tile([0.485, 0.456, 0.406], (B, 1)), np.tile([0.229, 0.224, 0.225], (B, 1))

    def one():
        loss = sum(model(imgs, tg, newMeans=means, newSTDs=stds).values())
        opt.zero_grad()
        loss.backward()
        opt.step()
    for _ in range(5):
        one()
    torch.cuda.synchronize()
    time.sleep(1.0)            # a gap in the kernel timeline: `report` counts what lies behind the last one (MIOpen's searches lie in front)
    t0 = time.perf_counter()
    for _ in range(10):
        one()
    torch.cuda.synchronize()
    print("%s: %.1f ms per step (host clock, 10 steps on a resident batch, under the tracer if one is attached)" % (mode, (time.perf_counter() - t0) * 100))


_MATRIX = ("igemm", "Cijk", "gemm", "Gemm", "conv", "Conv", "miopen", "Miopen", "MIOpen", "ck::", "naive", "SubTensor", "transpose", "Transpose", "Winograd",
           "winograd", "sp3", "asm_")
# forward + both gradients of body, FPN and the RPN head's 3x3 at b = 8, 800 x 1344 (an estimate from the layer shapes, not a count)
TRUNK_FLOP = 9.2e12


def report(dirs):
    """Device time of the ten timed steps: the kernels behind the last gap of >= 0.5 s in the trace (`steps` sleeps there; the
    warm-up steps in front of it hold MIOpen's searches for shapes the find-db has no record of)."""
    for d, name in zip(dirs, ("fp32", "--amp")):
        path = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[0]
        with open(path) as f:
            rows = list(csv.DictReader(f))
        kn = "Kernel_Name" if "Kernel_Name" in rows[0] else "Name"
        ev = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r[kn]) for r in rows), key=lambda e: e[0])
        cut, last_end = 0, ev[0][1]
        for i, (a, b, _) in enumerate(ev):
            if a - last_end >= 0.5e9:
                cut = i
            last_end = max(last_end, b)
        ev = ev[cut:]
        n_steps = 10
        per = {}
        for a, b, n in ev:
            t, c = per.get(n, (0.0, 0))
            per[n] = (t + (b - a) / 1e6, c + 1)
        fam = {"convolutions + GEMMs (MIOpen, hipBLASLt, their layout kernels)": 0.0, "dib_* kernels": 0.0, "everything else (ATen, ...)": 0.0}
        keys = list(fam)
        for n, (t, _) in per.items():
            k = keys[1] if "dib" in n else (keys[0] if any(s in n for s in _MATRIX) and "at::" not in n else keys[2])
            fam[k] += t
        total = sum(fam.values())
        print("%s: device time per step (the %d timed steps, %d kernels): %.1f ms; first to last kernel %.1f ms per step" % (
            name, n_steps, len(ev), total / n_steps, (max(e[1] for e in ev) - ev[0][0]) / 1e6 / n_steps))
        for k, v in fam.items():
            print("  %-70s %7.2f ms per step" % (k, v / n_steps))
        print("  convolutions + GEMMs at %.1f TFLOP per step: %.0f TFLOP/s" % (TRUNK_FLOP / 1e12, TRUNK_FLOP / (fam[keys[0]] / n_steps * 1e-3) / 1e12))
        print("  the 12 largest kernels (ms per step, calls per step, name):")
        for n, (t, c) in sorted(per.items(), key=lambda kv: -kv[1][0])[:12]:
            print("    %7.2f  %6.1f  %s" % (t / n_steps, c / n_steps, n[:140]))
        print("  dib_* trunk epilogues (us per call, calls per step, name):")
        for n, (t, c) in sorted(((n, v) for n, v in per.items() if "dib" in n and any(s in n for s in ("bias_act", "mask", "scatter", "topdown", "stem_pool", "fold", "scale_rows"))),
                                key=lambda kv: -kv[1][0]):
            print("    %8.1f  %6.1f  %s" % (t * 1e3 / c, c / n_steps, n[:110]))


def cell():
    from detectinblur_amd import evaluate as EV
    from detectinblur_amd import train as TR
    from detectinblur_amd import utils
    from detectinblur_amd.coco_utils import get_coco
    from detectinblur_amd.engine import evaluate
    dev = torch.device("cuda:0")
    model = _model(dev).eval()
    warm, n = 4, 16
    out = []
    for name, dt in (("fp32", torch.float32), ("--amp", BF), ("fp32 again", torch.float32)):
        model.backbone.compute_dtype = dt
        tf = TR.get_transform(False, blur=True, blur_type=EV.SWEEP_PARAMS[0], blur_ratio=1, blur_exposure=EV.SWEEP_FRACTIONS[0])
        ds, _ = get_coco(None, "val", tf, synthetic=dict(num_images=warm + n, size=(H, W)))
        loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, num_workers=0, collate_fn=utils.collate_fn, pin_memory=True)
        stamps = []

        def timed(it):
            for k, batch in enumerate(it):
                if k == warm:
                    torch.cuda.synchronize()
                    stamps.append(time.perf_counter())
                yield batch

        class L(object):
            dataset = ds

            def __iter__(self):
                return timed(iter(loader))

            def __len__(self):
                return len(loader)
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            evaluate(model, L(), device=dev, blurring_images=True, gpu_blur=True, expand_target_boxes=True)
        torch.cuda.synchronize()
        # the timed span ends after COCO accumulation of the cell, as the sweep's own wall clock does
        out.append("%s %.1f" % (name, n / (time.perf_counter() - stamps[0])))
    print("sweep cell P1E1, %d timed images after %d, images/s (COCO accumulation of the cell included): %s" % (n, warm, " | ".join(out)))


def convs():
    import torch.nn.functional as F
    from detectinblur_amd.models import backbone as BB
    from detectinblur_amd.models import rpn as R
    dev = torch.device("cuda:0")
    m = _model(dev).eval()
    m.backbone.compute_dtype = BF
    x = torch.randn(1, 3, 800, 1344, device=dev).contiguous(memory_format=torch.channels_last)
    calls, orig = [], BB.conv1x1

    def logged(x, w, b, conv):
        calls.append((tuple(x.shape), x.dtype, conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride))
        return orig(x, w, b, conv)
    BB.conv1x1 = R.conv1x1 = logged
    try:
        with torch.no_grad():
            m.rpn.head(list(m.backbone(x).values()))
    finally:
        BB.conv1x1 = R.conv1x1 = orig

    def timeit(fn, n=20):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n * 1000

    print("input shape, Cin -> Cout, kernel, stride | same bits in 5 runs: channels-last conv, detour | us: conv, detour (GEMM for 1x1, planar for 3x3), fp32 conv")
    seen = set()
    with torch.no_grad():
        for cfg in calls:
            shape, dt, ci, co, ks, st = cfg
            if cfg in seen or dt != BF:
                continue
            seen.add(cfg)
            xi = torch.randn(shape, device=dev).to(BF).contiguous(memory_format=torch.channels_last)
            w = (torch.randn(co, ci, *ks, device=dev) * 0.05).to(BF).contiguous(memory_format=torch.channels_last)
            pad = ks[0] // 2
            conv = lambda: F.conv2d(xi, w, None, st, pad)      # noqa: E731
            if ks == (1, 1):
                xs = xi if st == (1, 1) else xi[:, :, ::st[0], ::st[1]].contiguous(memory_format=torch.channels_last)
                w2 = w.reshape(co, ci)
                alt = lambda: F.linear(xs.permute(0, 2, 3, 1), w2).permute(0, 3, 1, 2)      # noqa: E731
            else:
                xp, wp = xi.contiguous(), w.contiguous()
                alt = lambda: F.conv2d(xp, wp, None, st, pad)      # noqa: E731
            det = []
            for fn in (conv, alt):
                ys = [fn().clone() for _ in range(5)]
                det.append(all(torch.equal(ys[0], y) for y in ys[1:]))
            x32, w32 = xi.float(), w.float()
            print("%-20s %4d -> %4d %s s%d | %-5s %-5s | %6.1f %6.1f %6.1f" % (shape, ci, co, "%dx%d" % ks, st[0], det[0], det[1], timeit(conv), timeit(alt),
                                                                             timeit(lambda: F.conv2d(x32, w32, None, st, pad))))
    # the stem: 3 -> 64, 7x7 / 2 on the image
    xi = torch.randn(1, 3, 800, 1344, device=dev).contiguous(memory_format=torch.channels_last)
    w = (torch.randn(64, 3, 7, 7, device=dev) * 0.05).contiguous(memory_format=torch.channels_last)
    xb, wb = xi.to(BF), w.to(BF)
    x8 = torch.randn(8, 3, 800, 1344, device=dev).contiguous(memory_format=torch.channels_last)
    x8b = x8.to(BF)
    with torch.no_grad():
        print("stem 7x7 / 2, 3 -> 64, us: b = 1 fp32 %.1f, bf16 %.1f; b = 8 fp32 %.1f, bf16 %.1f" % (
            timeit(lambda: F.conv2d(xi, w, None, 2, 3)), timeit(lambda: F.conv2d(xb, wb, None, 2, 3)),
            timeit(lambda: F.conv2d(x8, w, None, 2, 3)), timeit(lambda: F.conv2d(x8b, wb, None, 2, 3))))


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "train":
        train(int(sys.argv[2]) if len(sys.argv) > 2 else 30)
    elif mode == "steps":
        steps(sys.argv[2])
    elif mode == "report":
        report(sys.argv[2:4])
    elif mode == "cell":
        cell()
    elif mode == "convs":
        convs()
    else:
        raise SystemExit(__doc__)
