"""Measurements behind profiles/deblur_augment.txt (one MI355X): the trainer's saturation and noise augmentation
(--change_saturation, --patch_noise_sigma; csrc/dib_deblur_augment.hip).

    python scratch/deblur_augment_timing.py kernels     B = 16 patches of 256 x 256 from 480 x 640 Half images: dib_deblur_patches_augment,
                                                        dib_deblur_patches and augment_patches_torch on the same input, WARM + CALLS calls
                                                        each; prints a host clock per call (between two device synchronisations) and is
                                                        meant to run under `rocprofv3 --kernel-trace --stats` for the device times
    python scratch/deblur_augment_timing.py report DIR  device time per call from the *kernel_trace.csv under DIR
    python scratch/deblur_augment_timing.py ab          the trainer's step at its defaults with both flags on / off (off: the step as it was),
                                                        two trainers on the same batches, alternated three times behind a warm-up
"""
import csv
import glob
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deblur_train_timing as T      # noqa: E402  (setup, run_steps: the same batches and the same window as profiles/deblur_train.txt)

WARM, CALLS = 3, 20
B, PS, SIZE = 16, 256, (480, 640)


def kernels():
    import numpy as np
    import torch
    from detectinblur_amd.models import deblur_train as DT
    device = torch.device(os.environ.get("DIB_TIMING_DEVICE", "cuda"))      # cpu: a rehearsal of the plumbing, never a measurement
    sync = torch.cuda.synchronize if device.type == "cuda" else (lambda: None)
    g = torch.Generator().manual_seed(0)
    images = [torch.rand((3,) + SIZE, generator=g).half().to(device) for _ in range(B)]
    np.random.seed(0)
    import random
    random.seed(0)
    draws = [DT.draw_patch(SIZE[0], SIZE[1], PS, True, 2.0) for _ in range(B)]
    cases = (("dib_deblur_patches_augment (saturation + noise)", lambda: DT.augment_patches(images, draws, PS, True)),
             ("dib_deblur_patches_augment (saturation, sigma = 0)", lambda: DT.augment_patches(images, draws, PS, False)),
             ("dib_deblur_patches", lambda: DT.gather_patches(images, draws, PS)),
             ("augment_patches_torch, sigma = 0 (torch ops on the GPU)", lambda: DT.augment_patches_torch(images, draws, PS, False)))
    print("B = %d, ps = %d, %d x %d Half images; %d calls behind %d warm-up calls; rotated: %d of %d draws" %
          (B, PS, SIZE[0], SIZE[1], CALLS, WARM, sum(d.rot90 for d in draws), B))
    for name, fn in cases:
        for _ in range(WARM):
            fn()
        sync()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        sync()
        print("%-58s %9.1f us per call on the host clock (enqueue and device, whichever is longer)" % (name, (time.perf_counter() - t0) / CALLS * 1e6), flush=True)


def report(directory):
    """The phases run one after the other and each makes WARM + CALLS calls: the augment kernel's launches are split by order into the
    noise and the no-noise phase, every at::native kernel belongs to augment_patches_torch."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    if not rows:
        raise SystemExit("no *kernel_trace.csv under %s" % directory)
    rows.sort()
    n = WARM + CALLS
    aug = [d for _, d, name in rows if "patches_augment_kernel" in name]
    plain = [d for _, d, name in rows if "patches_kernel" in name]
    torch_side = [d for _, d, name in rows if "at::native" in name]
    assert len(aug) == 2 * n and len(plain) == n, (len(aug), len(plain))

    def line(what, d):
        d = d[WARM:]
        print("%-58s %8.2f us per launch: median (min %.2f, max %.2f) over %d launches" % (what, statistics.median(d) / 1e3, min(d) / 1e3, max(d) / 1e3, len(d)))

    line("patches_augment_kernel<Half>, saturation + noise", aug[:n])
    line("patches_augment_kernel<Half>, saturation, sigma = 0", aug[n:])
    line("patches_kernel<Half> x 3 channels (dib_deblur_patches)", plain)
    print("%-58s %8.2f us of device time per call, summed over %.1f torch kernels per call (%d calls, the warm-up's among them)"
          % ("augment_patches_torch, sigma = 0", sum(torch_side) / n / 1e3, len(torch_side) / n, n))
    moved = B * 3 * PS * PS * (2 + 4)
    print("bytes the augment launch needs: %.1f MB (Half in, fp32 out): %.2f TB/s at the no-noise median" % (moved / 1e6, moved / (statistics.median(aug[n + WARM:]) * 1e-9) / 1e12))


def ab(extra):
    flags = ["--change_saturation", "--patch_noise_sigma", "2"]
    cases = (("flags off (the step as it was)", []), ("--change_saturation --patch_noise_sigma 2", flags))
    trainers = []
    for _, f in cases:
        torch, args, trainer, batches = T.setup(list(extra) + f)
        trainers.append(trainer)
    times = [[] for _ in cases]
    for k, (name, _) in enumerate(cases):
        t0 = time.perf_counter()
        T.run_steps(torch, trainers[k], batches, T.WARM)
        print("warm-up, %-44s %.1f s for %d steps (path %s)" % (name, time.perf_counter() - t0, T.WARM, trainers[k].bare.last_path), flush=True)
    for rep in range(3):
        for k, (name, _) in enumerate(cases):
            dt, loss = T.run_steps(torch, trainers[k], batches, 6)
            times[k].append(dt)
            print("round %d  %-44s %.2f ms per step  %.1f images/s  (path %s, last loss %.3f)"
                  % (rep, name, dt * 1e3, args.batch_size / dt, trainers[k].bare.last_path, loss), flush=True)
    med = [statistics.median(t) for t in times]
    for k, (name, _) in enumerate(cases):
        t = times[k]
        print("%-44s median %.2f ms per step (min %.2f, max %.2f; spread %.2f %%)  %.1f images/s"
              % (name, med[k] * 1e3, min(t) * 1e3, max(t) * 1e3, 100 * (max(t) - min(t)) / med[k], args.batch_size / med[k]))
    print("flags on / flags off: %.4f x (ratio of medians), %+.2f ms per step" % (med[1] / med[0], (med[1] - med[0]) * 1e3))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "kernels":
        kernels()
    elif mode == "report":
        report(sys.argv[2])
    elif mode == "ab":
        ab(sys.argv[2:])
    else:
        raise SystemExit(__doc__)
