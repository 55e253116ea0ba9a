"""AugMix on the GPU: device time per kernel and train-step images/s with and without --non_pos_aug_mix (profiles/augmix.txt).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/nonpos -o am -- python scratch/augmix_timing.py kernels nonpos
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/pos -o am -- python scratch/augmix_timing.py kernels pos
    python scratch/augmix_timing.py report OUT/nonpos/am_kernel_stats.csv OUT/pos/am_kernel_stats.csv
    python scratch/augmix_timing.py train [steps]

`kernels`: 50 back-to-back calls of augmix.apply_plans_device on b = 8 images of 3 x 800 x 1333 with seeded plans (positional ops
or not).  `report`: each kernel's average device time from the trace against its algorithmic bytes (the same seeded plans) at
8 TB/s.  `train`: engine.train_one_epoch on Faster R-CNN, b = 8, synthetic 800 x 1333 images through the loader (8 workers),
--blur_train --gpu_blur --expand_target_boxes, without AugMix, with --non_pos_aug_mix and with --include_pos_aug_mix, alternated.
"""
import csv
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from detectinblur_amd import augmix as A  # noqa: E402

B, H, W = 8, 800, 1333


def plans(positional):
    np.random.seed(7 if positional else 3)
    return [A.draw_plan(H, W, positional)[0] for _ in range(B)]


def kernels(positional):
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(0)
    imgs = [torch.from_numpy(rs.randint(0, 256, (3, H, W)).astype(np.float32) / 255).to(dev) for _ in range(B)]
    ps = plans(positional)
    for _ in range(5):
        A.apply_plans_device(imgs, ps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        A.apply_plans_device(imgs, ps)
    torch.cuda.synchronize()
    print("%s: %.1f us per call (host clock, 50 calls)" % ("positional" if positional else "non-positional", (time.perf_counter() - t0) / 50 * 1e6))


def algorithmic_bytes(ps):
    """Bytes each kernel has to move (sum over launches of one call): fp32 input 12 B per pixel, uint8 stage images 3 B, fp16 out 6 B."""
    px = H * W
    nbytes = {"augmix_hist_kernel": B * px * 12, "augmix_lut_kernel": 0, "augmix_stage_kernel": 0, "augmix_mix_kernel": 0}
    for p in ps:
        npos = [sum(op in A.POSITIONAL_OPS for op, _ in chain) for chain in p["chains"]]
        for n in npos:
            for d in range(n):
                nbytes["augmix_stage_kernel"] += px * ((12 if d == 0 else 3) + 3)
        nbytes["augmix_mix_kernel"] += px * (12 + 3 * sum(1 for n in npos if n) + 6)
    return nbytes


def report(paths):
    for path, positional in zip(paths, (False, True)):
        ps = plans(positional)
        launches = {"augmix_hist_kernel": 1, "augmix_lut_kernel": 1 + max(sum(op in A.POSITIONAL_OPS for op, _ in c) for p in ps for c in p["chains"]),
                    "augmix_stage_kernel": max(sum(op in A.POSITIONAL_OPS for op, _ in c) for p in ps for c in p["chains"]), "augmix_mix_kernel": 1}
        need = algorithmic_bytes(ps)
        print("%s, b = %d at 3 x %d x %d (%d launches per call):" % ("positional ops" if positional else "non-positional ops", B, H, W,
                                                                    sum(launches.values())))
        total = 0.0
        if os.path.isdir(path):      # rocprofv3 may nest its files (host / process directories)
            import glob
            path = sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True))[0]
        with open(path) as f:
            rows = {r["Name"]: r for r in csv.DictReader(f)}
        for k in ("augmix_hist_kernel", "augmix_lut_kernel", "augmix_stage_kernel", "augmix_mix_kernel"):
            r = [v for n, v in rows.items() if k in n]
            if not r or launches[k] == 0:
                continue
            calls = int(r[0]["Calls"])
            us = float(r[0]["TotalDurationNs"]) / 1e3 / calls * launches[k]     # device time per AugMix call
            total += us
            frac = need[k] / (us * 1e-6) / 8e12 if need[k] else float("nan")
            print("  %-20s %8.1f us per call  %7.1f MB  %5.1f %% of 8 TB/s" % (k, us, need[k] / 1e6, 100 * frac))
        print("  %-20s %8.1f us per call" % ("total", total))


def train(steps):
    from detectinblur_amd import kernel_choices, utils
    from detectinblur_amd import train as TR
    from detectinblur_amd.coco_utils import get_coco
    from detectinblur_amd.engine import train_one_epoch
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    kernel_choices.use_shipped_kernel_choices()
    dev = torch.device("cuda:0")
    TR.seed_everything(False)
    model = fasterrcnn_resnet50_fpn(num_classes=91, pretrained=False, pretrained_backbone=False, trainable_backbone_layers=3).to(dev)
    opt = utils.make_sgd([p for p in model.parameters() if p.requires_grad], 0.0001, 0.9, 1e-4)
    warm = 5
    configs = {"no AugMix": {}, "--non_pos_aug_mix": {"non_pos_aug_mix": True},
               "--non_pos_aug_mix --include_pos_aug_mix --aug_mix_target_expand": {"non_pos_aug_mix": True, "include_pos_aug_mix": True,
                                                                                    "aug_mix_target_expand": True}}
    results = {k: [] for k in configs}
    for rep in range(3):
        for name, kw in configs.items():
            tf = TR.get_transform(True, blur=True, blur_ratio=0.9, defer_aug_mix=True, **kw)
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
            print("rep %d  %-62s %6.1f images/s" % (rep, name, ips), flush=True)
    base = np.median(results["no AugMix"])
    for name, v in results.items():
        print("median %-62s %6.1f images/s  (%+.1f %% vs no AugMix)  runs %s" % (name, np.median(v), 100 * (np.median(v) / base - 1),
                                                                               ", ".join("%.1f" % x for x in v)))


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "kernels":
        kernels(sys.argv[2] == "pos")
    elif mode == "report":
        report(sys.argv[2:4])
    else:
        train(int(sys.argv[2]) if len(sys.argv) > 2 else 30)
