"""Two versions of detectinblur_amd/engine.py under bench.py's evaluation sweep and loader-fed training epoch (profiles/eval_loop_refactor.txt).

    git show <commit>:detectinblur_amd/engine.py > /tmp/parent_engine.py
    for rep in 0 1 2; do for v in parent this; do
        python scratch/eval_loop_ab.py run $v out/${v}_$rep.json [--engine /tmp/parent_engine.py]      # --engine with `parent` only
    done; done
    python scratch/eval_loop_ab.py report out > profiles/eval_loop_refactor.txt

`run`: a fresh process per run -- bench.train_e2e_bench (16 steps behind 4; the model and optimiser from two train_step_bench steps
behind three) and bench.eval_sweep_bench (bench.py's default 16 timed images per cell, no amortised cell) -- with the given file in
place of the package's engine module, or the package's own.  `report`: the six runs, per figure the first version's range, its
spread, the range widened by that spread on either side, and whether each of the second version's runs lies inside."""
import glob
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run(variant, out_path, engine_file=None):
    import detectinblur_amd
    from detectinblur_amd import kernel_choices, utils
    utils.loader_context()                               # before this process touches the GPU, as bench.py --full does
    kernel_choices.use_shipped_kernel_choices()
    if engine_file is not None:
        spec = importlib.util.spec_from_file_location("detectinblur_amd.engine", engine_file)
        mod = importlib.util.module_from_spec(spec)
        sys.modules["detectinblur_amd.engine"] = mod
        spec.loader.exec_module(mod)
        detectinblur_amd.engine = mod
    from detectinblur_amd import engine
    import torch
    import bench
    t_start = time.perf_counter()
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    images, dicts, psfs, _host, _ = bench.make_workload(0, device, bench.make_psfs_host(0))
    _train, ddp, opt = bench.train_step_bench(images, dicts, psfs, device, None, 1, 0, 2, 3, account=False)
    e2e = bench.train_e2e_bench(ddp, opt, device, None, 1, 16, 4)
    del ddp, opt, images, psfs
    torch.cuda.empty_cache()
    t_e2e = time.perf_counter()
    sweep = bench.eval_sweep_bench(device, 16, None, 1, 0, 0)
    out = {"variant": variant, "engine_file": engine.__file__, "train_e2e": e2e["value"], "train_e2e_ms_per_step": e2e["ms_per_step"],
           "images_per_s": sweep["images_per_s"], "images_per_s_with_merge": sweep["images_per_s_with_merge"],
           "native_sizes": sweep["native_sizes"]["images_per_s"], "seconds": {"e2e": t_e2e - t_start, "sweep": time.perf_counter() - t_e2e}}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(out, f)
    print(json.dumps(out), flush=True)


def figures(run_):
    out = {"train_e2e": run_["train_e2e"]}
    for key in ("images_per_s", "images_per_s_with_merge"):
        for group, value in sorted(run_[key].items()):
            out["%s %s" % (key, group)] = value
    return out


def report(folder):
    runs = {}
    for path in sorted(glob.glob(os.path.join(folder, "*.json"))):
        r = json.load(open(path))
        runs.setdefault(r["variant"], []).append(figures(r))
    (first, a), (second, b) = sorted(runs.items())
    print("%-34s %-27s %-27s %7s  %-17s verdict" % ("figure (images/s)", first + " runs", second + " runs", "spread", "widened range"))
    inside_all, below = True, 0
    for name in a[0]:
        xs, ys = [r[name] for r in a], [r[name] for r in b]
        spread = max(xs) - min(xs)
        lo, hi = min(xs) - spread, max(xs) + spread
        inside = all(lo <= y <= hi for y in ys)
        inside_all = inside_all and inside
        below += sum(y < lo for y in ys)
        print("%-34s %-27s %-27s %7.2f  %7.2f - %7.2f inside" % (name, ", ".join("%.2f" % x for x in xs), ", ".join("%.2f" % y for y in ys), spread, lo, hi)
              if inside else
              "%-34s %-27s %-27s %7.2f  %7.2f - %7.2f OUTSIDE: %s" % (name, ", ".join("%.2f" % x for x in xs), ", ".join("%.2f" % y for y in ys), spread,
                                                                    lo, hi, ", ".join("%.2f (%s)" % (y, "below" if y < lo else "above")
                                                                                      for y in ys if not lo <= y <= hi)))
    print("every figure of `%s` inside `%s`'s range widened by its spread: %s; runs of `%s` BELOW that range: %d"
          % (second, first, "YES" if inside_all else "NO", second, below))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        engine_file = sys.argv[sys.argv.index("--engine") + 1] if "--engine" in sys.argv else None
        run(sys.argv[2], sys.argv[3], engine_file)
    else:
        report(sys.argv[2])
