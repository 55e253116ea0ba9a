"""Blur-estimator training driver -- reference train_blur_estimator.py (flags :511-585, loop :300-480).

ResNet-18 with a 16-way (or, with --LEHE_blur_seg, 4-way) head, trained on COCO images blurred on the
GPU by the same HIP path as the detector.  One process per GPU; `torchrun` / RANK, WORLD_SIZE,
LOCAL_RANK as in train.py.  Every flag of the reference's driver parses, with its default: AugMix (--non_pos_aug_mix, the pixels on
the GPU unless --cpu_blur) in the training transform, TensorBoard scalars under --tensorboard_path, --cpu_blur, the aspect-ratio
batch sampler, --pretrained from a locally cached file; the flags the reference parses and never reads are accepted and say so.

    python -m detectinblur_amd.train_blur_estimator --synthetic --blur_train --gpu_blur --crop_images --quantize_image \
        --non_pos_aug_mix --include_pos_aug_mix --tensorboard_path runs/estimator --output_dir weights/estimator -b 8
"""
import argparse
import datetime
import os
import time

import torch
from torch import nn

from . import utils
from .coco_utils import get_coco
from .engine_blur_estimator import evaluate, train_one_epoch
from .models.blur_estimator import resnet18
from .train import _seed_worker, add_blur_acc_mode_flag, get_transform, reject_idle_blur_acc_mode, seed_everything


def build_parser():
    p = argparse.ArgumentParser(description="detectInBlur hot path on MI355X: blur-estimator training")
    unused = " (parsed and never read, as in the reference)"
    p.add_argument("--dataset", default="coco")
    p.add_argument("--data_path", default=None)
    p.add_argument("--aspect-ratio-group-factor", default=3, type=int,
                   help="batches of images with similar aspect ratios (2 * k + 1 groups); a negative value: plain batches")
    p.add_argument("--synthetic", action="store_true", help="COCO-shaped synthetic data (no dataset on disk needed)")
    p.add_argument("--synthetic_images", default=64, type=int)
    p.add_argument("--synthetic_size", default=[480, 640], nargs=2, type=int)
    p.add_argument("--use_stored_psfs", action="store_true")
    p.add_argument("--stored_psf_directory", default=None)
    p.add_argument("--stored_psf_count", default=12000, type=int)
    p.add_argument("--crop_images", action="store_true", help="Crop images when batching.")
    p.add_argument("--resize_images", action="store_true")
    p.add_argument("--quantize_image", action="store_true")
    p.add_argument("--model", default="fasterrcnn_resnet50_fpn", help="model" + unused)
    p.add_argument("--trainable_backbone_blocks", default=3, type=int, help="Resnet backbone blocks to train." + unused)
    p.add_argument("--pretrained", action="store_true", help="Start from ImageNet ResNet-18 weights (a locally cached file; never downloaded).")
    p.add_argument("--device", default="cuda")
    p.add_argument("-b", "--batch_size", default=8, type=int)
    p.add_argument("-j", "--workers", default=0, type=int)
    p.add_argument("--lr", default=0.04, type=float)
    p.add_argument("--lr-step-size", default=8, type=int, help="decrease lr every step-size epochs" + unused)
    p.add_argument("--lr-steps", default=[16, 22], nargs="+", type=int)
    p.add_argument("--lr-gamma", default=0.1, type=float)
    p.add_argument("--epochs", default=37, type=int)
    p.add_argument("--momentum", default=0.9, type=float)
    p.add_argument("--wd", "--weight-decay", dest="weight_decay", default=1e-4, type=float)
    p.add_argument("--resume", default=None)
    p.add_argument("--start_from_weights", default=None)
    p.add_argument("--start_epoch", default=0, type=int)
    p.add_argument("--early_stop", type=int, default=None)
    p.add_argument("--eval_first", action="store_true")
    p.add_argument("--test_only", action="store_true")
    p.add_argument("--tensorboard_path", default="debug", help="directory of the TensorBoard event file (an empty string: none)")
    p.add_argument("--output_dir", default="debug")
    p.add_argument("--image_output_dir", default="debug", help="Output directory for images." + unused)
    p.add_argument("--print_freq", default=20, type=int)
    p.add_argument("--blur_train", action="store_true")
    p.add_argument("--cpu_blur", action="store_true", help="CPU blurring in the Fourier domain, in the data loader's workers.")
    p.add_argument("--gpu_blur", action="store_true")
    add_blur_acc_mode_flag(p)
    p.add_argument("--param_index", default=None)
    p.add_argument("--LEHE_blur_seg", action="store_true")
    p.add_argument("--high_exposure", action="store_true")
    p.add_argument("--low_exposure", action="store_true")
    p.add_argument("--expand_target_boxes", action="store_true", help="Expand target boxes according to blur kernel shifts." + unused)
    p.add_argument("--dont_center_psf", action="store_true")
    p.add_argument("--add_noise", action="store_true")
    p.add_argument("--noise_level", default=0.001, type=float)
    p.add_argument("--add_block", action="store_true")
    p.add_argument("--add_jpeg_artefacts", action="store_true")
    p.add_argument("--non_pos_aug_mix", action="store_true", help="Non positional augmix (training only; pixels on the GPU unless --cpu_blur).")
    p.add_argument("--include_pos_aug_mix", action="store_true", help="Include positional augmentations in augmix (with --non_pos_aug_mix).")
    p.add_argument("--aug_mix_target_expand", action="store_true",
                   help="Expand target boxes for AugMix according to positional shifts from spatial augmentations.")
    p.add_argument("--world-size", default=1, type=int)
    p.add_argument("--dist-url", default="env://")
    return p


def main(args):
    from . import kernel_choices
    kernel_choices.use_shipped_kernel_choices()      # shipped MIOpen / TunableOp choices, private copy per process (kernel_choices.py)
    reject_idle_blur_acc_mode(args)      # (this driver has no reject_out_of_scope: the same refusal, here)
    mp_ctx = utils.loader_context() if args.workers > 0 else None      # before anything touches the GPU (see utils.loader_context)
    utils.init_distributed_mode(args)
    print(args)
    seed_everything(args.distributed)
    device = torch.device(args.device if torch.cuda.is_available() or args.device == "cpu" else "cpu")
    if args.use_stored_psfs:
        blur_type = None if args.param_index is None else int(args.param_index)
    else:
        blur_type = None if args.param_index is None else [0.01, 0.005, 0.001, 0.00005][int(args.param_index)]
    blur_ratio = 0.75 if args.low_exposure else (1 if args.high_exposure else 0.9)
    writer = None
    if utils.is_main_process() and args.tensorboard_path:              # reference train_blur_estimator.py:128-139
        from .tb_writer import make_writer
        writer = make_writer(args.tensorboard_path)
    synthetic = dict(num_images=args.synthetic_images, size=tuple(args.synthetic_size), as_tensor=not args.cpu_blur) if args.synthetic else None
    common = dict(blur=True, blur_type=blur_type, blur_ratio=blur_ratio, use_stored_psfs=args.use_stored_psfs, cpu_blur=args.cpu_blur,
                  stored_psf_directory=args.stored_psf_directory, dont_center_psf=args.dont_center_psf,
                  low_exposure=args.low_exposure, high_exposure=args.high_exposure, stored_psf_count=args.stored_psf_count,
                  LEHE_blur_seg=args.LEHE_blur_seg)
    aug_mix = dict(non_pos_aug_mix=args.non_pos_aug_mix, include_pos_aug_mix=args.include_pos_aug_mix,       # :159-170: training only
                   aug_mix_target_expand=args.aug_mix_target_expand, defer_aug_mix=device.type == "cuda")
    dataset, _ = get_coco(args.data_path, "train", get_transform(True, **common, **aug_mix), synthetic=synthetic, with_masks=False)
    dataset_test, _ = get_coco(args.data_path, "val", get_transform(False, **common), synthetic=synthetic, with_masks=False)
    if args.distributed:
        train_sampler = torch.utils.data.distributed.DistributedSampler(dataset)
        test_sampler = torch.utils.data.distributed.DistributedSampler(dataset_test, shuffle=False)
    else:
        train_sampler = torch.utils.data.RandomSampler(dataset)
        test_sampler = torch.utils.data.SequentialSampler(dataset_test)
    if args.aspect_ratio_group_factor >= 0:                             # :192-198
        from .group_by_aspect_ratio import GroupedBatchSampler, create_aspect_ratio_groups
        batch_sampler = GroupedBatchSampler(train_sampler, create_aspect_ratio_groups(dataset, k=args.aspect_ratio_group_factor),
                                            args.batch_size)
    else:
        batch_sampler = torch.utils.data.BatchSampler(train_sampler, args.batch_size, drop_last=True)
    pin = device.type == "cuda"
    loader = torch.utils.data.DataLoader(dataset, batch_sampler=batch_sampler, num_workers=args.workers, collate_fn=utils.collate_fn,
                                         pin_memory=pin, worker_init_fn=_seed_worker, multiprocessing_context=mp_ctx)
    loader_test = torch.utils.data.DataLoader(dataset_test, batch_size=1, sampler=test_sampler,      # reference train_blur_estimator.py:206
                                              num_workers=args.workers, collate_fn=utils.collate_fn, pin_memory=pin,
                                              worker_init_fn=_seed_worker, multiprocessing_context=mp_ctx)

    print("Creating model")
    model = resnet18(pretrained=args.pretrained)                        # :212
    model.fc = nn.Linear(512, 4 if args.LEHE_blur_seg else 16)          # reference evaluate.py:188-194
    model = model.to(device).to(memory_format=torch.channels_last)
    bare = model
    if args.distributed:
        model = torch.nn.parallel.DistributedDataParallel(model, device_ids=[args.gpu] if device.type == "cuda" else None)
        bare = model.module
    criterion = nn.CrossEntropyLoss().to(device)
    optimizer = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=args.lr, momentum=args.momentum,
                                weight_decay=args.weight_decay)
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=args.lr_steps, gamma=args.lr_gamma)
    if args.resume:
        ck = torch.load(args.resume, map_location="cpu", weights_only=False)
        bare.load_state_dict(ck["model"]); optimizer.load_state_dict(ck["optimizer"]); scheduler.load_state_dict(ck["lr_scheduler"])
        args.start_epoch = ck["epoch"] + 1
    elif args.start_from_weights:
        bare.load_state_dict(torch.load(args.start_from_weights, map_location="cpu", weights_only=False)["model"])

    eval_kw = dict(device=device, distributed_mode=args.distributed, blurring_images=True, gpu_blur=args.gpu_blur,
                   LEHE_blur_seg=args.LEHE_blur_seg, resize_images=args.resize_images, quantize_image=args.quantize_image,
                   add_noise=args.add_noise, noise_level=args.noise_level, add_block=args.add_block,
                   add_jpeg_artifact=args.add_jpeg_artefacts, early_stop=args.early_stop, blur_acc_mode=args.blur_acc_mode)
    if args.eval_first or args.test_only:
        evaluate(model, loader_test, **eval_kw)
        if args.test_only:
            if writer is not None:
                writer.close()
            return
    print("Start training")
    start = time.time()
    for epoch in range(args.start_epoch, args.epochs):
        if args.distributed:
            train_sampler.set_epoch(epoch)
        train_one_epoch(model, optimizer, criterion, loader, device, args.print_freq, epoch, args.distributed, writer,
                        args.gpu_blur, args.LEHE_blur_seg, args.resize_images, args.quantize_image, args.crop_images,
                        args.add_noise, args.noise_level, args.add_block, args.add_jpeg_artefacts, args.early_stop, args.blur_train,
                        blur_acc_mode=args.blur_acc_mode)
        scheduler.step()
        if args.output_dir:
            utils.mkdir(args.output_dir)
            utils.save_on_master({"model": bare.state_dict(), "optimizer": optimizer.state_dict(),
                                  "lr_scheduler": scheduler.state_dict(), "args": args, "epoch": epoch},
                                 os.path.join(args.output_dir, "blur_estimator_{}.pth".format(epoch)))
        accuracies = evaluate(model, loader_test, **eval_kw)
        if writer is not None:                                          # :495-497
            writer.add_scalar("Blurred/Top1Accuracy", accuracies[0], epoch)
            writer.add_scalar("Blurred/Top2Accuracy", accuracies[1], epoch)
            writer.flush()
    if writer is not None:
        writer.close()
    print("Training time {}".format(str(datetime.timedelta(seconds=int(time.time() - start)))))


if __name__ == "__main__":
    main(build_parser().parse_args())
