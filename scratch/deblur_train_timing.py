"""Measurements behind profiles/deblur_train.txt (one MI355X).  The trainer's step -- GPU blur of a loader batch, patches, pyramids,
MSResNet forward, L1 loss, backward, Adam -- on loader batches drawn once and kept on the host (the loader itself, which draws the PSFs,
is not in the timed window), at the trainer's defaults unless flags say otherwise.

    python scratch/deblur_train_timing.py ab       FUSE_DEBLUR_TRAIN on / off alternated three times: step time, images/s
    python scratch/deblur_train_timing.py steps    a few fused steps behind a warm-up, to run under `rocprofv3 --kernel-trace --stats`
    python scratch/deblur_train_timing.py report DIR   sums the *_kernel_stats.csv under DIR by kernel family; where the per-dispatch
                                                   *_kernel_trace.csv is there, only the steps behind the warm-up (MIOpen's find, which
                                                   a fresh process repeats, stays out of the sums)
    python scratch/deblur_train_timing.py amp      fp32 as shipped / --amp on the HIP path / --amp under autocast, alternated three times
                                                   (profiles/deblur_train_amp.txt); `steps --amp` is the traced run behind it
"""
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, TRACED = 2, 3


def setup(extra=()):
    import torch
    from detectinblur_amd import kernel_choices, utils
    from detectinblur_amd import train_deblurrer as TD
    from detectinblur_amd.coco_utils import get_coco
    from detectinblur_amd.train import get_transform
    kernel_choices.use_shipped_kernel_choices()
    args = TD.build_parser().parse_args(["--synthetic", "--param_index", "1", "--low_exposure"] + list(extra))
    TD.reject(args)
    args.distributed = False
    device = torch.device(os.environ.get("DIB_TIMING_DEVICE", "cuda"))      # cpu: a rehearsal of the plumbing at a tiny size, never a measurement
    TD.seed_epoch(args.seed, 0)
    tf = get_transform(False, blur=True, blur_type=[0.01, 0.005, 0.001, 0.00005][int(args.param_index)], blur_ratio=0.75, low_exposure=True)
    dataset, _ = get_coco(None, "train", tf, synthetic=dict(num_images=args.synthetic_images, size=tuple(args.synthetic_size)), with_masks=False)
    batches = []
    for k in range(2):
        items = [dataset[k * args.batch_size + i] for i in range(args.batch_size)]
        batches.append(utils.collate_fn(items))
    trainer = TD.Trainer(args, device)
    return torch, args, trainer, batches


def run_steps(torch, trainer, batches, n):
    sync = torch.cuda.synchronize if trainer.device.type == "cuda" else (lambda: None)
    sync()
    t0 = time.perf_counter()
    for k in range(n):
        images, _, blur_dicts = batches[k % len(batches)]
        loss = trainer.step(images, blur_dicts)
    sync()
    return (time.perf_counter() - t0) / n, float(loss)


def ab(extra):
    from detectinblur_amd.models import deblur_train as DT
    torch, args, trainer, batches = setup(extra)
    print("defaults: -b %d --patch_size %d, %d scales x %d blocks x %d features, k %d; images %s; %d PSFs blurring in batch 0"
          % (args.batch_size, args.patch_size, args.n_scales, args.n_resblocks, args.n_feats, args.kernel_size, tuple(args.synthetic_size),
             sum(bd["blurring"] for bd in batches[0][2])))
    times = {True: [], False: []}
    for fuse in (True, False):
        DT.FUSE_DEBLUR_TRAIN = fuse
        t0 = time.perf_counter()
        run_steps(torch, trainer, batches, WARM)
        print("warm-up, fused %s: %.1f s for %d steps (path %s)" % (fuse, time.perf_counter() - t0, WARM, trainer.bare.last_path))
    for rep in range(3):
        for fuse in (True, False):
            DT.FUSE_DEBLUR_TRAIN = fuse
            dt, loss = run_steps(torch, trainer, batches, 6)
            times[fuse].append(dt)
            print("round %d  fused %-5s  %.2f ms per step  %.1f images/s  (path %s, last loss %.3f)"
                  % (rep, fuse, dt * 1e3, args.batch_size / dt, trainer.bare.last_path, loss))
    for fuse in (True, False):
        t = times[fuse]
        print("FUSE_DEBLUR_TRAIN %-5s  median %.2f ms per step (min %.2f, max %.2f)  %.1f images/s"
              % (fuse, statistics.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3, args.batch_size / statistics.median(t)))
    print("fused against plain: %.3f x (ratio of medians); spread of the rounds: fused %.1f %%, plain %.1f %%"
          % (statistics.median(times[False]) / statistics.median(times[True]),
             100 * (max(times[True]) - min(times[True])) / statistics.median(times[True]),
             100 * (max(times[False]) - min(times[False])) / statistics.median(times[False])))
    print("images left out at --patch_size %d on this data (--synthetic, every image %s): %d of %d"
          % (args.patch_size, tuple(args.synthetic_size), trainer.dropped, (2 * WARM + 36) * args.batch_size))
    if trainer.device.type == "cuda":
        print("peak device memory %.1f GB" % (torch.cuda.max_memory_allocated() / 2 ** 30))


def amp(extra):
    """Three trainers in one process on the same batches: fp32 as shipped, --amp with the Half HIP epilogues, --amp with the plain module
    under autocast (FUSE_DEBLUR_TRAIN = False).  The fp32 case is the baseline: the step as it stands without the flag."""
    from detectinblur_amd.models import deblur_train as DT
    shipped = DT.FUSE_DEBLUR_TRAIN, DT.FUSE_DEBLUR_TRAIN_AMP
    cases = (("fp32 as shipped", (), shipped), ("--amp, HIP epilogues", ("--amp",), (True, True)), ("--amp, autocast", ("--amp",), (False, False)))
    trainers, batches, torch, args = [], None, None, None
    for name, flags, _ in cases:
        torch, args, trainer, batches = setup(list(extra) + list(flags))
        trainers.append(trainer)
    rounds = int(os.environ.get("DIB_TIMING_STEPS", "6"))

    def select(k):
        DT.FUSE_DEBLUR_TRAIN, DT.FUSE_DEBLUR_TRAIN_AMP = cases[k][2]
        return trainers[k]

    times, peaks = [[] for _ in cases], [0.0] * len(cases)
    for k, (name, _, _) in enumerate(cases):
        t0 = time.perf_counter()
        run_steps(torch, select(k), batches, WARM)
        print("warm-up, %-22s %.1f s for %d steps (path %s)" % (name, time.perf_counter() - t0, WARM, trainers[k].bare.last_path), flush=True)
    for rep in range(3):
        for k, (name, _, _) in enumerate(cases):
            if trainers[k].device.type == "cuda":
                torch.cuda.reset_peak_memory_stats()
            dt, loss = run_steps(torch, select(k), batches, rounds)
            times[k].append(dt)
            if trainers[k].device.type == "cuda":
                peaks[k] = max(peaks[k], torch.cuda.max_memory_allocated() / 2 ** 30)
            scale = trainers[k].scaler.get_scale() if trainers[k].scaler is not None else float("nan")
            print("round %d  %-22s %.2f ms per step  %.1f images/s  (path %s, last loss %.3f, scale %g)"
                  % (rep, name, dt * 1e3, args.batch_size / dt, trainers[k].bare.last_path, loss, scale), flush=True)
    med = [statistics.median(t) for t in times]
    for k, (name, _, _) in enumerate(cases):
        t = times[k]
        print("%-22s median %.2f ms per step (min %.2f, max %.2f; spread %.1f %%)  %.1f images/s  peak memory of its rounds %.1f GB"
              % (name, med[k] * 1e3, min(t) * 1e3, max(t) * 1e3, 100 * (max(t) - min(t)) / med[k], args.batch_size / med[k], peaks[k]))
    print("fp32 / amp HIP %.3f x; fp32 / amp autocast %.3f x; amp autocast / amp HIP %.3f x (ratios of medians)"
          % (med[0] / med[1], med[0] / med[2], med[2] / med[1]))
    DT.FUSE_DEBLUR_TRAIN, DT.FUSE_DEBLUR_TRAIN_AMP = shipped


def steps(extra):
    from detectinblur_amd.models import deblur_train as DT
    torch, args, trainer, batches = setup(extra)
    DT.FUSE_DEBLUR_TRAIN = DT.FUSE_DEBLUR_TRAIN_AMP = True
    dt, _ = run_steps(torch, trainer, batches, WARM + TRACED)
    print("%d steps, %.2f ms per step under the tracer (warm-up included)" % (WARM + TRACED, dt * 1e3))


FAMILIES = (("(a) patches_kernel", ("patches_kernel",)), ("(b) bias_grad_partial + final", ("bias_grad_",)), ("(c) L1 loss: sliced_sum partial + final", ("L1Term", "l1_partial", "l1_final")),
            ("pyramid launches (deblur_level0 / deblur_down)", ("deblur_level0", "deblur_down")),
            ("bias_act forward epilogues", ("bias_act_kernel", "bias_act_f16_scalar")), ("the blur (blur_quad / blur_step / compaction)", ("blur_quad", "blur_step", "compact")))


def traced_steps_only(directory):
    """The per-dispatch trace (*kernel_trace.csv), cut at the first kernel of the first step behind the warm-up (every step begins with
    the blur's psf_compact launch) and summed by kernel name: the last TRACED steps without whatever MIOpen's find ran in the warm-up.
    None when the trace is not there or does not hold WARM + TRACED steps."""
    calls = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            calls.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    calls.sort()
    marks = [t0 for t0, _, name in calls if "psf_compact" in name]
    if len(marks) != WARM + TRACED:
        return None
    sums = {}
    for t0, t1, name in calls:
        if t0 >= marks[WARM]:
            c = sums.setdefault(name, [0, 0])
            c[0] += 1
            c[1] += t1 - t0
    return [{"Name": k, "Calls": c, "TotalDurationNs": t, "AverageNs": t / c} for k, (c, t) in sums.items()]


DIRECTIONS = (("weight gradients", ("_wrw_", "bwd_weight")), ("data gradients", ("_bwd_", "bwd_data")), ("forward", ("_fwd_", "conv_fwd")))


def report(directory):
    rows = traced_steps_only(directory)
    if rows is not None:
        print("from the per-dispatch trace: the %d steps behind the %d warm-up steps" % (TRACED, WARM))
        searching = sum(int(r["Calls"]) for r in rows if "naive_conv" in r["Name"])
        if searching:
            print("WARNING: %d launches of MIOpen's naive reference kernels in the traced steps: its find was still searching" % searching)
        return summarise(rows, TRACED, "")
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    for path in glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True) if not rows else ():
        # rocprofv3 without --output-format csv writes its rocpd database instead: the same sums from its `kernels` view
        import sqlite3
        for name, calls, total in sqlite3.connect(path).execute("select name, count(*), sum(duration) from kernels group by name"):
            rows.append({"Name": name, "Calls": calls, "TotalDurationNs": total, "AverageNs": total / calls})
    if not rows:
        raise SystemExit("no *kernel_stats.csv and no *_results.db under %s" % directory)
    summarise(rows, WARM + TRACED, ", the warm-up's among them")


def summarise(rows, n, note):
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    print("all kernels: %.2f ms of device time per step (%d kernels per step; %d steps%s)"
          % (total / n / 1e6, sum(int(r["Calls"]) for r in rows) // n, n, note))
    ours = 0.0
    for title, keys in FAMILIES:
        sel = [r for r in rows if "dib" in r["Name"] and any(k in r["Name"] for k in keys)]
        t = sum(float(r["TotalDurationNs"]) for r in sel)
        calls = sum(int(r["Calls"]) for r in sel)
        ours += t
        print("  %-50s %9.1f us per step  %5d launches per step  %5.2f %%" % (title, t / n / 1e3, calls // n, 100 * t / total))
    torch_side = [r for r in rows if "at::native" in r["Name"]]
    tt = sum(float(r["TotalDurationNs"]) for r in torch_side)
    print("  %-50s %9.1f us per step  %5d launches per step  %5.2f %%" % ("torch's own kernels (at::native: Adam, cat, copies)", tt / n / 1e3,
                                                                         sum(int(r["Calls"]) for r in torch_side) // n, 100 * tt / total))
    rest = total - ours - tt
    print("  %-50s %9.1f us per step  %27s  %5.2f %%" % ("everything else: MIOpen's convolution kernels", rest / n / 1e3, "", 100 * rest / total))
    others = [r for r in rows if "dib" not in r["Name"] and "at::native" not in r["Name"]]
    for title, keys in DIRECTIONS:
        sel = [r for r in others if any(k in r["Name"] for k in keys)]
        others = [r for r in others if r not in sel]
        t = sum(float(r["TotalDurationNs"]) for r in sel)
        print("    %-48s %9.1f us per step  %5d launches per step  %5.2f %%" % ("of which " + title, t / n / 1e3, sum(int(r["Calls"]) for r in sel) // n,
                                                                             100 * t / total))
    print("the ten largest:")
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:10]:
        print("  %6.2f %%  %6d calls  %9.1f us each  %s" % (100 * float(r["TotalDurationNs"]) / total, int(r["Calls"]), float(r["AverageNs"]) / 1e3, r["Name"][:110]))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "ab"
    if mode == "ab":
        ab(sys.argv[2:])
    elif mode == "amp":
        amp(sys.argv[2:])
    elif mode == "steps":
        steps(sys.argv[2:])
    elif mode == "report":
        report(sys.argv[2])
    else:
        raise SystemExit(__doc__)
