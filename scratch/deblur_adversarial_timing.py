"""Measurements behind profiles/deblur_adversarial.txt (one MI355X): the trainer's adversarial loss (--loss 1*L1+1*ADV;
models/deblur_adversarial.py, csrc/dib_deblur_adv.hip).

    python scratch/deblur_adversarial_timing.py ab          the trainer's step at its defaults, fp32 and then --amp: --loss 1*L1 (the step as it
                                                            was), 1*L1+1*ADV with FUSE_DEBLUR_ADV on, and the same trainer with it off (the plain
                                                            module); alternated four times behind a warm-up, the order reversed in every other
                                                            round, on the same batches
    python scratch/deblur_adversarial_timing.py steps       WARM + TRACED steps with ADV, fp32 and then --amp, FUSE_DEBLUR_ADV on: meant to run under
                                                            `rocprofv3 --kernel-trace --output-format csv` for the new kernels' device time
    python scratch/deblur_adversarial_timing.py report DIR  device time of the new kernels per step from the *kernel_trace.csv under DIR
"""
import csv
import glob
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deblur_train_timing as T      # noqa: E402  (setup, run_steps: the same batches and the same window as profiles/deblur_train.txt)

ADV = ["--loss", "1*L1+1*ADV"]
STEPS = int(os.environ.get("DIB_TIMING_STEPS", "4"))
ROUNDS = 4


def ab(extra):
    from detectinblur_amd.models import deblur_adversarial as DA
    for precision in ([], ["--amp"]):
        torch, args, plain, batches = T.setup(list(extra) + precision)
        _, _, adv, _ = T.setup(list(extra) + precision + ADV)
        cases = (("--loss 1*L1 (the step as it was)", plain, True), ("--loss 1*L1+1*ADV, FUSE_DEBLUR_ADV on", adv, True),
                 ("--loss 1*L1+1*ADV, FUSE_DEBLUR_ADV off", adv, False))
        print("== %s" % ("--amp" if precision else "fp32"))
        for name, trainer, fuse in cases:
            DA.FUSE_DEBLUR_ADV = fuse
            t0 = time.perf_counter()
            T.run_steps(torch, trainer, batches, T.WARM)
            print("warm-up, %-42s %.1f s for %d steps (path %s, d_path %s)"
                  % (name, time.perf_counter() - t0, T.WARM, trainer.bare.last_path, trainer.bare_d.last_path if trainer.bare_d is not None else "-"), flush=True)
        times = [[] for _ in cases]
        for rep in range(ROUNDS):
            # the order is reversed in every other round: the two ADV cases share a trainer, and neither always runs behind the other
            for k, (name, trainer, fuse) in (list(enumerate(cases)) if rep % 2 == 0 else list(enumerate(cases))[::-1]):
                DA.FUSE_DEBLUR_ADV = fuse
                dt, loss = T.run_steps(torch, trainer, batches, STEPS)
                times[k].append(dt)
                print("round %d  %-42s %.2f ms per step  (d_path %s, last loss %.3f)"
                      % (rep, name, dt * 1e3, trainer.bare_d.last_path if trainer.bare_d is not None else "-", loss), flush=True)
        med = [statistics.median(t) for t in times]
        for k, (name, _, _) in enumerate(cases):
            t = times[k]
            print("%-42s median %.2f ms per step (min %.2f, max %.2f; spread %.2f %%)  %.1f images/s"
                  % (name, med[k] * 1e3, min(t) * 1e3, max(t) * 1e3, 100 * (max(t) - min(t)) / med[k], args.batch_size / med[k]))
        print("ADV on / L1 alone: %.4f x, %+.2f ms per step;  FUSE_DEBLUR_ADV off / on: %.4f x, %+.2f ms per step"
              % (med[1] / med[0], (med[1] - med[0]) * 1e3, med[2] / med[1], (med[2] - med[1]) * 1e3), flush=True)
        del plain, adv
        if torch.cuda.is_available():
            torch.cuda.empty_cache()


def steps(extra):
    from detectinblur_amd.models import deblur_adversarial as DA
    DA.FUSE_DEBLUR_ADV = True
    for precision in ([], ["--amp"]):
        torch, args, trainer, batches = T.setup(list(extra) + precision + ADV)
        dt, _ = T.run_steps(torch, trainer, batches, T.WARM + T.TRACED)
        print("%s: %d steps, %.2f ms per step under the tracer (warm-up included; d_path %s)"
              % ("--amp" if precision else "fp32", T.WARM + T.TRACED, dt * 1e3, trainer.bare_d.last_path), flush=True)
        del trainer


FAMILIES = (("leaky_fwd_kernel<F32Lane, mask>", ("leaky_fwd_kernel", "F32Lane")), ("leaky_bwd_kernel<F32Lane>", ("leaky_bwd_kernel", "F32Lane")),
            ("leaky_fwd_kernel<F16Lane, mask>", ("leaky_fwd_kernel", "F16Lane")), ("leaky_bwd_kernel<F16Lane>", ("leaky_bwd_kernel", "F16Lane")),
            ("BCE loss: sliced_sum partial + final (both precisions)", ("BceTerm|adv_bce_",)))      # (a|b: the name before the kernels were shared)


def report(directory):
    """The new kernels run in every step alike and are no part of MIOpen's search: all WARM + TRACED steps of each precision are summed."""
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            rows.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    if not rows:
        raise SystemExit("no *kernel_trace.csv under %s" % directory)
    n = T.WARM + T.TRACED
    for title, keys in FAMILIES:
        d = [t for t, name in rows if all(any(a in name for a in k.split("|")) for k in keys)]
        if not d:
            print("%-66s no launch in the trace" % title)
            continue
        per = n * (2 if "both" in title else 1)
        print("%-66s %8.1f us per step in %5.1f launches per step; per launch median %.2f us (min %.2f, max %.2f)"
              % (title, sum(d) / per / 1e3, len(d) / per, statistics.median(d) / 1e3, min(d) / 1e3, max(d) / 1e3))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "ab":
        ab(sys.argv[2:])
    elif mode == "steps":
        steps(sys.argv[2:])
    elif mode == "report":
        report(sys.argv[2])
    else:
        raise SystemExit(__doc__)
