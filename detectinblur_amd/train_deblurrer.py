"""DeepDeblur trainer: the blind "deblur, then detect" baseline's network, trained on (blurred, sharp) pairs that the GPU blur makes.

The reference vendors DeepDeblur's trainer beside its inference wrapper (models/deblur/train.py, dataCommon.py, model.py); this is
this project's, and what it writes is what `evaluate.py --deblur_first --deblurer_model_location DIR` loads.

    python -m detectinblur_amd.train_deblurrer --synthetic --param_index 1 --low_exposure --output_dir weights/deblur -b 16

One step: sharp images from the loader (COCO or --synthetic; the `BlurImage` transform and `collate_fn` of train.py draw the PSFs),
blurred on the GPU by `blur_image_list` (--gpu_blur is implied; --cpu_blur is refused), the sharp originals kept; one random patch
per image cut from both with the same draws and the same augmentation (models/deblur_train.py: the draw order of the reference's
dataCommon.py); both quantised to 8 bits and built into Gaussian pyramids; MSResNet forward; the multi-scale L1 loss; backward;
Adam.  The host reads the loss only every --print_freq steps: the step itself does not synchronise.

Defaults are DeepDeblur's published ones (-b 16, --patch_size 256, --lr 1e-4, Adam (0.9, 0.999), --lr-steps 500 750 900, --lr-gamma
0.5, --epochs 1000, 3 scales x 19 blocks x 64 features, 5 x 5 kernels, loss sum_s mean |out_s - target_s|, fp32).  Its option.py and
loss/ are not in the reference tree: a STATED READING, not pinned.  Not built: bf16 training, a batched pyramid kernel, tuned
convolution choices.  No accuracy or PSNR claim is made anywhere: synthetic data shows nothing.

--loss (the reference's deblurInterface.py:184, default 1*L1): terms weight*NAME joined by +, names in either case; L1 and ADV are
built, anything else is refused at start.  With the default the step is call for call what it was, no discriminator is constructed
and the checkpoint stays {"G"}.  With ADV the reference's discriminator (models/deblur_adversarial.py; discriminator.py, built by
model.py:31-34 whenever --loss contains adv) is trained beside the generator; --patch_size must be at least 193.  One step with ADV --
like L1's, a STATED READING: DeepDeblur's loss/ package is not in the reference tree:
    G forward as before; fake = finest output + 127.5, real = finest target + 127.5 (0..255, channels-last; Half under --amp);
    D update:  opt_D.zero_grad; loss_d = BCE(D(fake.detach()), 0) + BCE(D(real), 1), one device scalar; backward; opt_D steps;
    G update:  loss_g = BCE(D(fake), 1) through the unwrapped discriminator with its parameters' requires_grad off (no weight-gradient
               convolutions, DistributedDataParallel's reducer not involved); total = w_L1 * L1 + w_ADV * loss_g; backward; opt_G steps.
opt_D is Adam with G's lr, betas and fusedness and a MultiStepLR of its own on the same milestones.  Under --amp one GradScaler serves
both: scale(loss_d).backward(); step(opt_D); scale(total).backward(); step(opt_G); update().  Nothing in the step reads the device.
model-<N>.pt becomes {"G", "D"} (the reference's layout; `Deblurer` reads "G"), optim-<N>.pt gains optimizer_D and lr_scheduler_D, and
--resume refuses a file written with another --loss.  Not built: other loss terms, more than one D update per step, fake and real
through D as one batch, tuned records for D's convolutions, a Half loss kernel.

--change_saturation and --patch_noise_sigma S: the value half of dataCommon.py's recipe (augment's HSV saturation change :72-87; add_noise
:43-54, DeepDeblur's S is 2), off by default.  Per image one factor uniform(0.5, 1.5) scales the saturation of both patches, and the
blurred patch alone gets Gaussian noise of sigma normal() * S grey levels; both ride in the patch launch (models/deblur_train.py,
"values"; csrc/dib_deblur_augment.hip).  With neither flag the step is call for call what it was.  --validate_images stays unaugmented.

--amp (the reference's train.py:43-46, 97-103, deblurInterface.py:144-145): the mixed-precision step.  Half input pyramids and Half
convolutions on fp32 master weights (models/deblur_train.py, "MIXED PRECISION"), the loss in fp32 on the upcast outputs, against fp32
targets; `torch.amp.GradScaler(init_scale=--init_scale)` around a FUSED Adam, which takes the scaler's found_inf and scale on the
device: a step with a non-finite gradient is skipped and the scale halved without the host reading anything.  The printed loss is the
unscaled one; the scale is read, with the loss, every --print_freq steps.  The checkpoint stays fp32; optim-<N>.pt gains "scaler".

Small images: an image with a side below --patch_size is left out of its step's batch; the count is printed per epoch.

Checkpoints: <output_dir>/models/model-<epoch>.pt holds {"G": state_dict} (epochs count from 1), the layout `Deblurer` loads
strictly.  Optimizer and scheduler state go to <output_dir>/optim/optim-<epoch>.pt, never under models/: `find_checkpoint` takes the
LAST name of a string sort of that directory (model-9.pt sorts after model-10.pt), and a warning is printed when the epoch about to
be written is not the one it would pick.  --resume (optionally with an optim file) continues from the last epoch saved; every epoch
reseeds the host generators with --seed + epoch, so a resumed run draws what the uninterrupted run draws.

--validate_images K: after each saved epoch, K held-out images are blurred with a fixed seed and `Deblurer(output_dir).deblur_` -- the
shipped inference path, on the checkpoint `find_checkpoint` picks -- is compared with the sharp image: its PSNR beside the PSNR of
the blurred input, and the SSIM of both (quality.py), to stdout and TensorBoard.

On --device cpu (tests, debugging) the network, the patches and the pyramid take their torch paths and the blur is a plain fp32
torch convolution with the same PSF: a stand-in, not the HIP blur's arithmetic."""
import argparse
import datetime
import math
import os
import random
import re
import time

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import utils
from .coco_utils import get_coco
from .train import _seed_worker, add_blur_acc_mode_flag, get_transform, reject_idle_blur_acc_mode


def build_parser():
    p = argparse.ArgumentParser(description="detectInBlur on MI355X: DeepDeblur training on pairs from the GPU blur")
    p.add_argument("--dataset", default="coco")
    p.add_argument("--data_path", default=None)
    p.add_argument("--synthetic", action="store_true", help="COCO-shaped synthetic data (no dataset on disk needed)")
    p.add_argument("--synthetic_images", default=64, type=int)
    p.add_argument("--synthetic_size", default=[480, 640], nargs=2, type=int)
    p.add_argument("--device", default="cuda")
    p.add_argument("-b", "--batch_size", default=16, type=int)
    p.add_argument("-j", "--workers", default=0, type=int)
    p.add_argument("--patch_size", default=256, type=int)
    p.add_argument("--lr", default=1e-4, type=float)
    p.add_argument("--lr-steps", default=[500, 750, 900], nargs="+", type=int)
    p.add_argument("--lr-gamma", default=0.5, type=float)
    p.add_argument("--epochs", default=1000, type=int)
    p.add_argument("--n_scales", default=3, type=int)
    p.add_argument("--n_resblocks", default=19, type=int)
    p.add_argument("--n_feats", default=64, type=int)
    p.add_argument("--kernel_size", default=5, type=int)
    p.add_argument("--output_dir", default="debug")
    p.add_argument("--resume", nargs="?", const="", default=None, metavar="OPTIM_FILE",
                   help="continue from <output_dir>/optim/optim-<N>.pt (the highest N, or the file given) and models/model-<N>.pt beside it")
    p.add_argument("--tensorboard_path", default="", help="directory of the TensorBoard event file (an empty string: none)")
    p.add_argument("--early_stop", type=int, default=None, help="leave an epoch once more than this many steps have run")
    p.add_argument("--print_freq", default=20, type=int, help="the host reads (and prints) the loss every this many steps")
    p.add_argument("--seed", default=1337, type=int)
    p.add_argument("--save_every", default=10, type=int, help="epochs between checkpoints (the last epoch is always saved)")
    p.add_argument("--validate_images", default=0, type=int, metavar="K")
    p.add_argument("--amp", action="store_true", help="mixed precision: Half convolutions on fp32 master weights, loss scaling")
    p.add_argument("--init_scale", default=DEFAULT_INIT_SCALE, type=float, help="--amp: the loss scale GradScaler starts from")
    p.add_argument("--loss", default=DEFAULT_LOSS, help="terms weight*NAME joined by + (the reference's grammar); built: L1, ADV (the adversarial "
                                                        "loss: trains the reference's discriminator beside the generator)")
    p.add_argument("--change_saturation", action="store_true",
                   help="dataCommon.augment's change_saturation: S of both patches scaled by one uniform(0.5, 1.5) factor per image")
    p.add_argument("--patch_noise_sigma", default=0.0, type=float, metavar="S",
                   help="dataCommon.add_noise's sigma_sigma (DeepDeblur: 2), on the blurred patch only; 0: off.  Not --add_noise, which "
                        "belongs to the blur stage")
    # the blur: the flags of train.py that the GPU blur reads
    p.add_argument("--gpu_blur", action="store_true", help="implied: the pairs are made by the GPU blur")
    p.add_argument("--cpu_blur", action="store_true", help="refused: the loader's FFT blur would leave no sharp original on the device")
    add_blur_acc_mode_flag(p)
    p.add_argument("--param_index", default=None)
    p.add_argument("--low_exposure", action="store_true")
    p.add_argument("--high_exposure", action="store_true")
    p.add_argument("--use_stored_psfs", action="store_true")
    p.add_argument("--stored_psf_directory", default=None)
    p.add_argument("--stored_psf_count", default=12000, type=int)
    p.add_argument("--dont_center_psf", action="store_true")
    p.add_argument("--add_noise", action="store_true")
    p.add_argument("--noise_level", default=0.001, type=float)
    p.add_argument("--add_block", action="store_true")
    p.add_argument("--add_jpeg_artefacts", action="store_true")
    p.add_argument("--world-size", default=1, type=int)
    p.add_argument("--dist-url", default="env://")
    return p


DEFAULT_INIT_SCALE = 1024.0      # the reference's (deblurInterface.py:145)
DEFAULT_LOSS = "1*L1"            # the reference's (deblurInterface.py:184)
LOSS_NAMES = ("L1", "ADV")


def parse_loss(spec):
    """--loss -> {NAME: weight} in the order given.  The reference's grammar (terms weight*NAME joined by +), names in either case;
    every refusal names the offending part."""
    if not str(spec).strip():
        raise SystemExit("--loss %r: needs at least one of %s, as weight*NAME" % (spec, " and ".join(LOSS_NAMES)))
    out = {}
    for term in str(spec).split("+"):
        part = term.strip()
        weight, star, name = part.partition("*")
        if not star or not weight.strip():
            raise SystemExit("--loss %s: the term %r has no weight; write weight*NAME, as in %s" % (spec, part, DEFAULT_LOSS))
        try:
            w = float(weight)
        except ValueError:
            raise SystemExit("--loss %s: the weight %r of the term %r is not a number" % (spec, weight.strip(), part))
        if not (math.isfinite(w) and w > 0):
            raise SystemExit("--loss %s: the weight %r of the term %r needs to be finite and above 0" % (spec, weight.strip(), part))
        key = name.strip().upper()
        if key not in LOSS_NAMES:
            raise SystemExit("--loss %s: the loss %r is not built; %s are" % (spec, name.strip(), " and ".join(LOSS_NAMES)))
        if key in out:
            raise SystemExit("--loss %s: %s is given twice" % (spec, key))
        out[key] = w
    return out


def reject_idle_init_scale(args):
    """--init_scale without --amp would be silently ignored: refuse it."""
    if not args.amp and args.init_scale != DEFAULT_INIT_SCALE:
        raise SystemExit("--init_scale %g: the loss scale belongs to --amp, which is not given; drop the flag or add --amp" % args.init_scale)
    if args.amp and not (math.isfinite(args.init_scale) and args.init_scale > 0):
        raise SystemExit("--init_scale %g: needs a finite scale above 0" % args.init_scale)


def reject(args):
    if args.cpu_blur:
        raise SystemExit("--cpu_blur: the deblurrer trains on pairs made by the GPU blur (the loader's FFT blur hands over no sharp "
                         "original); drop the flag")
    d = 2 ** (args.n_scales - 1)
    if args.n_scales < 1 or args.patch_size < d or args.patch_size % d:
        raise SystemExit("--patch_size %d is not a multiple of 2 ** (n_scales - 1) = %d: the pyramid halves it n_scales - 1 times"
                         % (args.patch_size, d))
    args.gpu_blur = True
    reject_idle_blur_acc_mode(args)
    reject_idle_init_scale(args)
    if "ADV" in parse_loss(args.loss):
        from .models.deblur_adversarial import min_side
        if args.patch_size < min_side(args.kernel_size):
            raise SystemExit("--loss %s with --patch_size %d: the discriminator's strides (2, 2, 4, 4, then a 4 x 4 convolution) need a patch "
                             "of at least %d" % (args.loss, args.patch_size, min_side(args.kernel_size)))
    if not (math.isfinite(args.patch_noise_sigma) and args.patch_noise_sigma >= 0):
        raise SystemExit("--patch_noise_sigma %g: needs a finite level of at least 0 (0: no noise)" % args.patch_noise_sigma)
    if "coco" not in args.dataset:
        raise SystemExit("--dataset %s: only COCO (and --synthetic) is built" % args.dataset)


def seed_epoch(seed, epoch, rank=0):
    """Every epoch starts from host generators seeded with --seed + epoch (+ 1337 * rank): what --resume relies on."""
    s = (seed + epoch + 1337 * rank) % 2 ** 31
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


class AdvNet(nn.Module):
    """The discriminator behind `discriminator_forward`, as a module so that DistributedDataParallel sees the forward."""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, x):
        from .models.deblur_adversarial import discriminator_forward
        return discriminator_forward(self.model, x)


class TrainNet(nn.Module):
    """MSResNet behind `msresnet_train_forward`, as a module so that DistributedDataParallel sees the forward."""

    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, *levels):
        from .models.deblur_train import msresnet_train_forward
        return tuple(msresnet_train_forward(self.model, list(levels)))


def blur_host(images, blur_dicts):
    """--device cpu only: images[i] replaced by an fp32 torch convolution with its normalised PSF (reflect padding where the image is
    large enough for it, zero padding otherwise).  A stand-in for tests, not the HIP blur's arithmetic."""
    for i, bd in enumerate(blur_dicts):
        if not bd["blurring"]:
            continue
        psf = torch.as_tensor(np.asarray(bd["psf"], dtype=np.float32))
        psf = (psf / psf.sum()).flip(0, 1)[None, None]
        K = psf.shape[-1]
        x = images[i].float()[:, None]
        pad = (K // 2 - 1, K // 2, K // 2 - 1, K // 2)
        x = F.pad(x, pad, mode="reflect") if min(x.shape[-2:]) > K // 2 else F.pad(x, pad)
        images[i] = F.conv2d(x, psf)[:, 0].clamp_(0, 1).to(images[i].dtype)


def make_pairs(images_CPU, blur_dicts, device, args, jpeg=None):
    """(blurred, sharp): two lists of Half [3, H, W] images on `device`."""
    from .blur_ops import acc_mode_constant
    from .engine_blur_estimator import _post, _stage
    from .models import blur_functions
    cuda = device.type == "cuda"
    images, _, psfs, tables = _stage(images_CPU, [], blur_dicts, device, True, cuda, args.blur_acc_mode)
    sharp = list(images)
    if cuda:
        blur_functions.blur_image_list(images, blur_dicts, psfs, args.add_noise, args.noise_level, args.add_block, args.add_jpeg_artefacts,
                                       jpeg, acc_mode=acc_mode_constant(args.blur_acc_mode), tables=tables)
    else:
        blur_host(images, blur_dicts)
        images = _post(images, args.add_noise, args.noise_level, args.add_block, False, jpeg)
    return images, sharp


class Trainer(object):
    """Model, optimizer and one training step; `step` never synchronises with the device."""

    def __init__(self, args, device):
        from .models.deblur import MSResNet
        self.args, self.device = args, device
        torch.manual_seed(args.seed)
        bare = MSResNet(n_scales=args.n_scales, n_resblocks=args.n_resblocks, n_feats=args.n_feats, kernel_size=args.kernel_size).to(device)
        if device.type == "cuda":
            bare = bare.to(memory_format=torch.channels_last)
        self.bare = bare
        self.net = TrainNet(bare)
        if getattr(args, "distributed", False):
            self.net = torch.nn.parallel.DistributedDataParallel(self.net, device_ids=[args.gpu] if device.type == "cuda" else None)
        self.loss_weights = parse_loss(args.loss)
        self.bare_d = self.net_d = self.optimizer_d = self.scheduler_d = self.last_adv = None
        if "ADV" in self.loss_weights:
            # after G, so that G's initial weights are those of a run without ADV
            from .models.deblur_adversarial import Discriminator
            self.bare_d = Discriminator(n_feats=args.n_feats, kernel_size=args.kernel_size).to(device)
            if device.type == "cuda":
                self.bare_d = self.bare_d.to(memory_format=torch.channels_last)
            self.net_d = AdvNet(self.bare_d)
            if getattr(args, "distributed", False):
                self.net_d = torch.nn.parallel.DistributedDataParallel(self.net_d, device_ids=[args.gpu] if device.type == "cuda" else None)
        self.scaler = None
        if args.amp:
            # fused: the scaler hands found_inf and the scale to the optimizer's kernel (`_step_supports_amp_scaling`); any other Adam
            # has the scaler read found_inf on the host every step
            self.optimizer = torch.optim.Adam(bare.parameters(), lr=args.lr, betas=(0.9, 0.999), fused=True)
            self.scaler = torch.amp.GradScaler(device.type, init_scale=args.init_scale)
        else:
            self.optimizer = torch.optim.Adam(bare.parameters(), lr=args.lr, betas=(0.9, 0.999))
        self.scheduler = torch.optim.lr_scheduler.MultiStepLR(self.optimizer, milestones=args.lr_steps, gamma=args.lr_gamma)
        if self.bare_d is not None:
            # G's lr, betas and fusedness; a schedule of its own on the same milestones
            fused = dict(fused=True) if args.amp else {}
            self.optimizer_d = torch.optim.Adam(self.bare_d.parameters(), lr=args.lr, betas=(0.9, 0.999), **fused)
            self.scheduler_d = torch.optim.lr_scheduler.MultiStepLR(self.optimizer_d, milestones=args.lr_steps, gamma=args.lr_gamma)
        self.jpeg = None
        if args.add_jpeg_artefacts:
            from .engine_blur_estimator import _jpeg
            self.jpeg = _jpeg(device)
        self.dropped = 0

    def step(self, images_CPU, blur_dicts):
        """One step on a loader batch -> the loss (a 0-dim tensor on the device), or None when no image of the batch is large enough."""
        from .models import deblur_train as DT
        ps = self.args.patch_size
        keep = [i for i, im in enumerate(images_CPU) if im.shape[-2] >= ps and im.shape[-1] >= ps]
        self.dropped += len(images_CPU) - len(keep)
        if not keep:
            if getattr(self.args, "distributed", False):
                raise RuntimeError("no image of this rank's batch has both sides >= --patch_size %d: the ranks' steps would part" % ps)
            return None
        blurred, sharp = make_pairs([images_CPU[i] for i in keep], [blur_dicts[i] for i in keep], self.device, self.args, self.jpeg)
        amp = self.scaler is not None
        if self.args.change_saturation or self.args.patch_noise_sigma:
            # dataCommon's augment on both patches with one factor, add_noise on the blurred one only (a stated reading: DESIGN.md 4)
            draws = [DT.draw_patch(int(im.shape[-2]), int(im.shape[-1]), ps, self.args.change_saturation, self.args.patch_noise_sigma)
                     for im in sharp]
            inputs = DT.patch_levels(DT.augment_patches(blurred, draws, ps, True), self.args.n_scales, torch.float16 if amp else torch.float32)
            targets = DT.patch_levels(DT.augment_patches(sharp, draws, ps, False), self.args.n_scales)
        else:
            draws = [DT.draw_patch(int(im.shape[-2]), int(im.shape[-1]), ps) for im in sharp]
            inputs = DT.patch_levels(DT.gather_patches(blurred, draws, ps), self.args.n_scales, torch.float16 if amp else torch.float32)
            targets = DT.patch_levels(DT.gather_patches(sharp, draws, ps), self.args.n_scales)
        outputs = list(self.net(*inputs))
        if self.bare_d is not None:
            return self._step_adversarial(outputs, targets, amp)
        loss = DT.pyramid_l1_loss([o.float() for o in outputs] if amp else outputs, targets)
        w = self.loss_weights["L1"]
        if w != 1.0:
            loss = loss * w
        self.optimizer.zero_grad(set_to_none=True)
        if amp:
            self.scaler.scale(loss).backward()
            self.scaler.step(self.optimizer)
            self.scaler.update()
        else:
            loss.backward()
            self.optimizer.step()
        return loss.detach()

    def _step_adversarial(self, outputs, targets, amp):
        """The rest of a step with ADV in --loss (the module docstring, "One step with ADV"): the D update on the detached fake, then the
        G update through the unwrapped discriminator with its parameters' requires_grad off.  `last_adv`: (loss_g, loss_d, the unweighted L1
        term -- a zero where --loss has none), on the device."""
        from .models import deblur_adversarial as DA
        from .models import deblur_train as DT
        fake = (outputs[0] + 127.5).contiguous(memory_format=torch.channels_last)
        real = targets[0][:, :3] + 127.5
        real = (real.half() if amp else real).contiguous(memory_format=torch.channels_last)
        self.optimizer_d.zero_grad(set_to_none=True)
        loss_d = DA.discriminator_loss(self.net_d, fake, real)
        if amp:
            self.scaler.scale(loss_d).backward()
            self.scaler.step(self.optimizer_d)
        else:
            loss_d.backward()
            self.optimizer_d.step()
        for p in self.bare_d.parameters():
            p.requires_grad_(False)
        try:
            loss_g = DA.adv_bce(DA.discriminator_forward(self.bare_d, fake).float(), 1)
            total, l1 = self.loss_weights["ADV"] * loss_g, None
            if "L1" in self.loss_weights:
                l1 = DT.pyramid_l1_loss([o.float() for o in outputs] if amp else outputs, targets)
                total = total + self.loss_weights["L1"] * l1
            self.optimizer.zero_grad(set_to_none=True)
            if amp:
                self.scaler.scale(total).backward()
                self.scaler.step(self.optimizer)
                self.scaler.update()
            else:
                total.backward()
                self.optimizer.step()
        finally:
            for p in self.bare_d.parameters():
                p.requires_grad_(True)
        self.last_adv = (loss_g.detach(), loss_d.detach(), l1.detach() if l1 is not None else torch.zeros_like(total))
        return total.detach()


def _epoch_of(name):
    m = re.search(r"-(\d+)\.pt$", name)
    return int(m.group(1)) if m else None


def warn_if_not_picked(models_dir, epoch):
    """`find_checkpoint` takes the last name of a STRING sort of models/: says so when that will not be the epoch about to be written."""
    new = "model-%d.pt" % epoch
    names = sorted(set(os.listdir(models_dir) if os.path.isdir(models_dir) else []) | {new})
    if names[-1] != new:
        print("WARNING: %s is written, but `Deblurer` / --deblurer_model_location on this directory will load %s: find_checkpoint takes "
              "the last name of a string sort (model-9.pt sorts after model-10.pt); point it at the file instead" % (new, names[-1]))
        return True
    return False


def save(trainer, args, epoch):
    """epoch: 1-based, the number of finished epochs."""
    models_dir, optim_dir = os.path.join(args.output_dir, "models"), os.path.join(args.output_dir, "optim")
    if utils.is_main_process():
        utils.mkdir(models_dir)
        utils.mkdir(optim_dir)
        warn_if_not_picked(models_dir, epoch)
    model = {"G": trainer.bare.state_dict()}
    if trainer.bare_d is not None:
        model["D"] = trainer.bare_d.state_dict()      # the reference's layout (model.py: Model.state_dict)
    utils.save_on_master(model, os.path.join(models_dir, "model-%d.pt" % epoch))
    state = {"optimizer": trainer.optimizer.state_dict(), "lr_scheduler": trainer.scheduler.state_dict(), "epoch": epoch, "args": vars(args)}
    if trainer.bare_d is not None:
        state["optimizer_D"] = trainer.optimizer_d.state_dict()
        state["lr_scheduler_D"] = trainer.scheduler_d.state_dict()
    if trainer.scaler is not None:
        state["scaler"] = trainer.scaler.state_dict()
    utils.save_on_master(state, os.path.join(optim_dir, "optim-%d.pt" % epoch))


def resume(trainer, args):
    """-> the number of epochs already done"""
    path = args.resume
    if not path:
        optim_dir = os.path.join(args.output_dir, "optim")
        epochs = [e for e in map(_epoch_of, os.listdir(optim_dir) if os.path.isdir(optim_dir) else []) if e is not None]
        if not epochs:
            raise SystemExit("--resume: no optim-<N>.pt under %s" % optim_dir)
        path = os.path.join(optim_dir, "optim-%d.pt" % max(epochs))
    ck = torch.load(path, map_location="cpu", weights_only=False)
    was_amp = bool(ck.get("args", {}).get("amp", False))
    if was_amp != bool(args.amp):
        raise SystemExit("--resume: %s was written %s --amp and this run is %s it: the optimizer state (and the loss scale) of one does "
                         "not continue the other; %s the flag" % (path, "with" if was_amp else "without", "with" if args.amp else "without",
                                                                  "add" if was_amp else "drop"))
    was_loss = ck.get("args", {}).get("loss", DEFAULT_LOSS)
    if parse_loss(was_loss) != parse_loss(args.loss):
        raise SystemExit("--resume: %s was written with --loss %s and this run is with --loss %s: the optimizer state (and the "
                         "discriminator) of one does not continue the other; give --loss %s" % (path, was_loss, args.loss, was_loss))
    model_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(path))), "models", "model-%d.pt" % ck["epoch"])
    model = torch.load(model_path, map_location="cpu", weights_only=True)
    trainer.bare.load_state_dict(model["G"], strict=True)
    if trainer.bare_d is not None:
        trainer.bare_d.load_state_dict(model["D"], strict=True)
        trainer.optimizer_d.load_state_dict(ck["optimizer_D"])
        trainer.scheduler_d.load_state_dict(ck["lr_scheduler_D"])
    trainer.optimizer.load_state_dict(ck["optimizer"])
    trainer.scheduler.load_state_dict(ck["lr_scheduler"])
    if trainer.scaler is not None:
        trainer.scaler.load_state_dict(ck["scaler"])
    print("Resumed from %s and %s" % (path, model_path))
    return int(ck["epoch"])


def psnr(a, b):
    mse = torch.mean((a.float() - b.float()) ** 2).item()
    return float("inf") if mse == 0 else 10.0 * math.log10(1.0 / mse)


def _planar(image):
    """what quality.psnr_ssim takes: contiguous, Half or fp32"""
    image = image if image.dtype in (torch.float16, torch.float32) else image.float()
    return image if image.is_contiguous() else image.contiguous()


@torch.no_grad()
def validate(dataset, args, device, K):
    """K held-out images blurred with a fixed seed, through the shipped inference path on the directory just written -> (mean PSNR of
    the deblurred image, mean PSNR of the blurred input, mean SSIM of the deblurred image, mean SSIM of the blurred input, number of
    images the SSIMs are over: those with both sides of at least 11 pixels), all against the sharp image.  The PSNRs are `psnr`'s; the SSIMs are quality.psnr_ssim's (one HIP pass per pair on a GPU), kept on the device and
    read once behind the loop.  The host generators are left as found."""
    from . import quality
    from .models.deblur import Deblurer
    states = random.getstate(), np.random.get_state(), torch.get_rng_state()
    try:
        seed_epoch(args.seed, 10 ** 6)
        deblurer = Deblurer(args.output_dir, device=device)
        out, inp, n, ssims = 0.0, 0.0, 0, []
        for i in range(min(K, len(dataset))):
            image, _, bd = dataset[i]
            blurred, sharp = make_pairs([image], [bd], device, args)
            deblurred = deblurer.deblur_(blurred[0])
            out += psnr(deblurred, sharp[0])
            inp += psnr(blurred[0], sharp[0])
            n += 1
            if min(sharp[0].shape[-2:]) >= quality.TAPS:      # (a side below the 11-pixel window has no SSIM)
                # one pass for both: the sharp image is read once (bit for bit the two psnr_ssim calls it replaces)
                ssims.append(quality.restoration_quality(_planar(sharp[0]), [_planar(deblurred), _planar(blurred[0])])[2::3])
        ssim_out, ssim_inp = torch.stack(ssims).double().mean(0).tolist() if ssims else (float("nan"), float("nan"))
        return (out / n, inp / n, ssim_out, ssim_inp, len(ssims)) if n else (float("nan"),) * 4 + (0,)
    finally:
        random.setstate(states[0])
        np.random.set_state(states[1])
        torch.set_rng_state(states[2])


def main(argv=None):
    args = build_parser().parse_args(argv)
    reject(args)
    from . import kernel_choices
    kernel_choices.use_shipped_kernel_choices()      # the trainer's own shapes are not in the shipped set: they run on MIOpen's find
    mp_ctx = utils.loader_context() if args.workers > 0 else None      # before anything touches the GPU (see utils.loader_context)
    utils.init_distributed_mode(args)
    print(args)
    rank = utils.get_rank()
    device = torch.device(args.device if torch.cuda.is_available() or args.device == "cpu" else "cpu")
    if args.use_stored_psfs:
        blur_type = None if args.param_index is None else int(args.param_index)
    else:
        blur_type = None if args.param_index is None else [0.01, 0.005, 0.001, 0.00005][int(args.param_index)]
    blur_ratio = 0.75 if args.low_exposure else (1 if args.high_exposure else 0.9)
    writer = None
    if utils.is_main_process() and args.tensorboard_path:
        from .tb_writer import make_writer
        writer = make_writer(args.tensorboard_path)
    synthetic = dict(num_images=args.synthetic_images, size=tuple(args.synthetic_size)) if args.synthetic else None
    common = dict(blur=True, blur_type=blur_type, blur_ratio=blur_ratio, use_stored_psfs=args.use_stored_psfs, cpu_blur=False,
                  stored_psf_directory=args.stored_psf_directory, dont_center_psf=args.dont_center_psf, low_exposure=args.low_exposure,
                  high_exposure=args.high_exposure, stored_psf_count=args.stored_psf_count)
    # no RandomHorizontalFlip: the patch augmentation flips
    dataset, _ = get_coco(args.data_path, "train", get_transform(False, **common), synthetic=synthetic, with_masks=False)
    dataset_val = None
    if args.validate_images > 0:
        val_synthetic = dict(synthetic, seed=4242) if synthetic else None      # held out: other images than the training set's
        dataset_val, _ = get_coco(args.data_path, "val", get_transform(False, **common), synthetic=val_synthetic, with_masks=False)
    seed_epoch(args.seed, 0, rank)
    if args.distributed:
        sampler = torch.utils.data.distributed.DistributedSampler(dataset)
    else:
        sampler = torch.utils.data.RandomSampler(dataset)
    loader = torch.utils.data.DataLoader(dataset, batch_size=args.batch_size, sampler=sampler, drop_last=True, num_workers=args.workers,
                                         collate_fn=utils.collate_fn, pin_memory=device.type == "cuda", worker_init_fn=_seed_worker,
                                         multiprocessing_context=mp_ctx)
    print("Creating model")
    trainer = Trainer(args, device)
    done = resume(trainer, args) if args.resume is not None else 0

    print("Start training")
    start = time.time()
    for epoch in range(done, args.epochs):
        seed_epoch(args.seed, epoch, rank)
        if args.distributed:
            sampler.set_epoch(epoch)
        trainer.dropped, it, seen, t0 = 0, 0, 0, time.time()
        for images_CPU, _targets, blur_dicts in loader:
            loss = trainer.step(images_CPU, blur_dicts)
            seen += len(images_CPU)
            if loss is not None and it % args.print_freq == 0:
                adv = trainer.last_adv
                if adv is None:
                    value = loss.item()              # the only read of the step's result: every --print_freq steps
                else:
                    value, adv_g, adv_d, l1 = torch.stack((loss,) + adv).tolist()      # ... with ADV: the scalars in one read
                line = "Epoch: [%d]  [%d/%d]  loss: %.4f  lr: %.6g  path: %s" % (epoch + 1, it, len(loader), value,
                                                                                  trainer.optimizer.param_groups[0]["lr"], trainer.bare.last_path)
                if adv is not None:
                    line += "  adv: %.4f  d: %.4f  d_path: %s" % (adv_g, adv_d, trainer.bare_d.last_path)
                if trainer.scaler is not None:
                    line += "  scale: %g" % trainer.scaler.get_scale()      # a read of the device, like the loss's: only here
                print(line)
                if writer is not None:
                    step = it + epoch * len(loader)
                    # the printed loss is the weighted total; this tag holds the L1 term itself, unweighted, with or without ADV
                    if "L1" in trainer.loss_weights:
                        writer.add_scalar("losses/l1_pyramid", value / trainer.loss_weights["L1"] if adv is None else l1, step)
                    if adv is not None:
                        writer.add_scalar("losses/adv_g", adv_g, step)
                        writer.add_scalar("losses/adv_d", adv_d, step)
                    writer.add_scalar("learningRate", trainer.optimizer.param_groups[0]["lr"], step)
                if not all(math.isfinite(v) for v in ((value,) if adv is None else (value, adv_g, adv_d))):
                    raise SystemExit("Loss is %r, stopping training" % (value if adv is None else (value, adv_g, adv_d),))
            it += 1
            if args.early_stop is not None and it > args.early_stop:
                break
        trainer.scheduler.step()
        if trainer.scheduler_d is not None:
            trainer.scheduler_d.step()
        print("Epoch: [%d] done: %d steps, %d images, %d left out (a side below --patch_size %d), %.1f s"
              % (epoch + 1, it, seen, trainer.dropped, args.patch_size, time.time() - t0))
        if args.output_dir and ((epoch + 1) % args.save_every == 0 or epoch + 1 == args.epochs):
            save(trainer, args, epoch + 1)
            if dataset_val is not None and utils.is_main_process():
                out, inp, ssim_out, ssim_inp, n_ssim = validate(dataset_val, args, device, args.validate_images)
                print("Validation: [%d]  PSNR deblurred %.2f dB, blurred input %.2f dB; SSIM deblurred %.4f, blurred input %.4f "
                      "(%d images, SSIM over %d of them; no quality claim)"
                      % (epoch + 1, out, inp, ssim_out, ssim_inp, min(args.validate_images, len(dataset_val)), n_ssim))
                if writer is not None:
                    writer.add_scalar("Validation/PSNR_deblurred", out, epoch + 1)
                    writer.add_scalar("Validation/PSNR_blurred_input", inp, epoch + 1)
                    writer.add_scalar("Validation/SSIM_deblurred", ssim_out, epoch + 1)
                    writer.add_scalar("Validation/SSIM_blurred_input", ssim_inp, epoch + 1)
            if writer is not None:
                writer.flush()
    if writer is not None:
        writer.close()
    print("Training time {}".format(str(datetime.timedelta(seconds=int(time.time() - start)))))
    return trainer


if __name__ == "__main__":
    main()
