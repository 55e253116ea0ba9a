"""Evaluation driver with the reference's hot-path flags (reference evaluate.py:378-468): one detector,
or the 4-detector ensemble routed per image by a ResNet-18 blur estimator (`--use_ensemble`, `--LEHE`)
or by the ground-truth blur_dict, over the blur sweep P in {0.005, 0.001, 0.00005} x E in
{1/25, 1/10, 1/5, 1/2, 1} (reference evaluate.py:299-370).  Image-parallel across ranks with a
DistributedSampler, batch size 1 per rank as in the reference.  `--vanilla_eval` scores clean images once
(reference :226-262).  Every pass returns the reference's CocoEvaluator surface and logs its statistics to
TensorBoard under the reference's tags.  Random-initialised models stand in for checkpoints when no paths are
given (synthetic throughput runs).  The reference README's command lines parse unchanged.
`--save_images` (this repo) writes the reference's detection overlays (reference engine.py:382-383) under `--image_output_dir`: one
subfolder per pass -- `clean` for the vanilla pass, `P<param>_E<fraction>` for each sweep cell (the reference hands every pass the
same folder, so its 15 cells overwrite one another's img<count>.png; and it always writes, where this needs the flag).
`--deblur_first --deblurer_model_location DIR` puts DeepDeblur's MSResNet in front of the detector in every pass (reference
evaluate.py:240-243, engine.py:319-322; models/deblur.py): the image stays on the device from the blur to the detector.
`--deblur_precision half` runs that stage as DeepDeblur's `--precision half` does (the module and its pyramid in Half) and hands the
detector a Half image; `--amp` is independent of it and leaves the deblurrer alone.
`--acclimate_norm` (this repo's flag for the reference layer's `acclimation_mode`, models/batchnorm.py:142-157, and the helpers of
its utils.py:80-217): online batch-norm statistics, updated on the device image by image (models/batchnorm.py, engine.evaluate).
`--deconvolve_first` (this repo): Richardson-Lucy deconvolution with the image's own, known PSF in front of the detector in every sweep
cell (models/deconvolve.py; `--deconvolve_iterations N`): the non-blind upper bound next to `--deblur_first`'s blind baseline.
`--deconvolve_tv LAMBDA` (this repo) adds the total-variation prior of Dey et al. 2006 to every iteration (beta = 1e-2)."""
import os
import argparse

import torch
import torch.utils.data
from torch import nn

from . import utils
from .coco_utils import get_coco
from .engine import evaluate
from .models.blur_estimator import resnet18
from .models.faster_rcnn import fasterrcnn_resnet50_fpn
from .train import _seed_worker, add_shared_flags, detector_size_kwargs, get_transform, log_coco_stats, reject_out_of_scope, seed_everything

SWEEP_PARAMS = [0.005, 0.001, 0.00005]
SWEEP_FRACTIONS = [1 / 25, 1 / 10, 1 / 5, 1 / 2, 1]
ACCLIMATION_PRIOR = 16
DECONVOLVE_ITERATIONS, MAX_DECONVOLVE_ITERATIONS = 30, 1000      # models/deconvolve.py's DEFAULT_ITERATIONS / MAX_ITERATIONS
MAX_DECONVOLVE_TV, DECONVOLVE_TV_BETA = 0.1, 1e-2                # models/deconvolve.py's MAX_TV_LAMBDA / DEFAULT_TV_BETA


def build_parser():
    """reference evaluate.py:378-466, flag for flag (shared ones in train.add_shared_flags)."""
    p = add_shared_flags(argparse.ArgumentParser(description="detectInBlur hot path on MI355X: evaluation"))
    p.set_defaults(synthetic_images=32)
    p.add_argument("--use_ensemble", action="store_true", help="Use blur network system ensemble.")
    p.add_argument("--ensemble_model_paths", default=None, nargs="+", help="Ensemble model paths (one quoted string or several).")
    p.add_argument("--blur_estimator_path", default=None, help="Blur estimator model path.")
    p.add_argument("--use_blur_estimator", action="store_true", help="(this repo) route with a random-init estimator when no path is given")
    p.add_argument("--vanilla_eval", action="store_true", help="Vanilla eval on clean COCO images.")
    p.add_argument("--blur_eval", action="store_true", help="Blur during evaluation (the sweep always blurs, as in the reference).")
    p.add_argument("--LEHE", action="store_true", help="System with low and high exposure networks.")
    p.add_argument("--dilate_psf", action="store_true", help="Dilate PSF to simulate defocus with motion blur.")
    p.add_argument("--model_path", default=None, help="(this repo) alias of --resume")
    p.add_argument("--save_images", action="store_true", help="(this repo) write every evaluated image with its detections above 0.5 "
                   "as <image_output_dir>/<pass>/img<count>.png (<pass>: clean, or P<param>_E<fraction> per sweep cell)")
    # outside the built path: accepted, refused when set
    p.add_argument("--blurred_dataset", action="store_true", help="(not built) real-blur datasets")
    p.add_argument("--expand_synth_boxes", action="store_true", help="(not built) real-blur datasets")
    p.add_argument("--mode_one_norm", action="store_true", help="Test-time batch-norm: every layer mixes the image's statistics "
                   "into its running ones (single model only, as in the reference)")
    p.add_argument("--acclimate_norm", action="store_true", help="(this repo) Online batch-norm statistics, the reference layer's "
                   "acclimation_mode: every layer folds the image's statistics into its running ones, on the device, and normalises "
                   "with the updated ones; the detector drifts toward the stream it sees (single model, fp32)")
    p.add_argument("--acclimation_momentum", type=float, default=None, help="(this repo) with --acclimate_norm: the exponential "
                   "average's factor; unset: the cumulative average over --acclimation_prior + images seen")
    p.add_argument("--acclimation_prior", type=int, default=None, help="(this repo) with --acclimate_norm: the batches the source "
                   "statistics count for (default %d: the first image weighs 1/%d, as in --mode_one_norm)" % (ACCLIMATION_PRIOR, ACCLIMATION_PRIOR + 1))
    p.add_argument("--acclimation_carry_over", action="store_true", help="(this repo) with --acclimate_norm: the statistics run on "
                   "through the passes (the 15 sweep cells) instead of starting every pass from the source statistics")
    p.add_argument("--deconvolve_first", action="store_true", help="(this repo) Deconvolve every blurred image with its own, known PSF "
                   "(Richardson-Lucy on the blur's forward model, on the device) before detecting: the non-blind upper bound of "
                   "--deblur_first.  Needs --gpu_blur.  With --expand_target_boxes the ground truth is still grown for the blurred image")
    p.add_argument("--deconvolve_iterations", type=int, default=DECONVOLVE_ITERATIONS, metavar="N", action=_StoreGiven, help="(this repo) with --deconvolve_first: "
                   "Richardson-Lucy iterations, 1..%d (default %d); more sharpen further and amplify noise and JPEG residue further"
                   % (MAX_DECONVOLVE_ITERATIONS, DECONVOLVE_ITERATIONS))
    p.add_argument("--deconvolve_tv", type=float, default=None, metavar="LAMBDA", help="(this repo) with --deconvolve_first: total-variation "
                   "regularised Richardson-Lucy (Dey et al. 2006), one factor per pixel and iteration that keeps the iteration from "
                   "amplifying noise, block and JPEG residue.  LAMBDA in (0, %g]; 0.002 to 0.01 is the working range, larger values "
                   "flatten detail.  beta is 1e-2.  Unset: the plain iteration" % MAX_DECONVOLVE_TV)
    p.add_argument("--restoration_metrics", action="store_true", help="(this repo) Per sweep cell, PSNR and SSIM of the blurred image and "
                   "of what --deblur_first / --deconvolve_first makes of it, against the image before the blur (quality.py; one HIP pass "
                   "per image, accumulated on the device).  Needs --gpu_blur.  No accuracy claim")
    p.add_argument("--restoration_8bit", action="store_true", help="(this repo) with --restoration_metrics: score the images as their "
                   "8-bit grey levels (data range 255), as figures computed from saved pictures are")
    return p


class _StoreGiven(argparse.Action):
    """stores the value and notes, as <dest>_given, that the flag was on the command line (its default says nothing about that)"""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        setattr(namespace, self.dest + "_given", True)


def reject_deconvolution_conflicts(args):
    """--deconvolve_first's refusals, before anything is built."""
    n = getattr(args, "deconvolve_iterations", DECONVOLVE_ITERATIONS)
    tv = getattr(args, "deconvolve_tv", None)
    if not getattr(args, "deconvolve_first", False):
        if getattr(args, "deconvolve_iterations_given", False):
            raise SystemExit("--deconvolve_iterations needs --deconvolve_first: it is the iteration count of that stage and nothing else "
                             "reads it")
        if tv is not None:
            raise SystemExit("--deconvolve_tv needs --deconvolve_first: it is the prior of that stage's iteration and nothing else reads it")
        return
    if getattr(args, "deblur_first", False):
        raise SystemExit("--deconvolve_first with --deblur_first: both replace the image in front of the detector (the blind network "
                         "and the known-PSF iteration); choose one")
    if getattr(args, "vanilla_eval", False):
        raise SystemExit("--deconvolve_first with --vanilla_eval: the clean pass has no PSF, the flag would do nothing")
    if getattr(args, "cpu_blur", False) or not getattr(args, "gpu_blur", False):
        raise SystemExit("--deconvolve_first needs --gpu_blur (and not --cpu_blur): the iteration inverts the sparse correlation of "
                         "--gpu_blur; the FFT path of --cpu_blur rescales every image to its own minimum and maximum, which is not "
                         "that forward model")
    if not (1 <= n <= MAX_DECONVOLVE_ITERATIONS):
        raise SystemExit("--deconvolve_iterations %d: the iteration count lies in 1..%d" % (n, MAX_DECONVOLVE_ITERATIONS))
    if tv is not None and not (0 < tv <= MAX_DECONVOLVE_TV):
        raise SystemExit("--deconvolve_tv %g: lambda lies in (0, %g] (0.002 to 0.01 is the working range; without the flag the iteration "
                         "is the plain one)" % (tv, MAX_DECONVOLVE_TV))


def reject_restoration_metrics_conflicts(args):
    """--restoration_metrics' refusals, before anything is built."""
    if not getattr(args, "restoration_metrics", False):
        if getattr(args, "restoration_8bit", False):
            raise SystemExit("--restoration_8bit needs --restoration_metrics: it sets how those figures are computed and nothing else reads it")
        return
    if getattr(args, "vanilla_eval", False):
        raise SystemExit("--restoration_metrics with --vanilla_eval: the clean pass blurs nothing, there is no image to compare with the "
                         "sharp one")
    if getattr(args, "cpu_blur", False) or not getattr(args, "gpu_blur", False):
        raise SystemExit("--restoration_metrics needs --gpu_blur (and not --cpu_blur): the sharp image is kept where the blur runs, right "
                         "before the blur replaces it; --cpu_blur blurs in the loaders' transform and hands the driver no sharp image")


def build_deconvolver(args):
    """the Deconvolver of `--deconvolve_first` with `--deconvolve_iterations` and `--deconvolve_tv`, or None"""
    if not getattr(args, "deconvolve_first", False):
        return None
    from .models.deconvolve import Deconvolver
    tv = getattr(args, "deconvolve_tv", None)
    return Deconvolver(iterations=getattr(args, "deconvolve_iterations", DECONVOLVE_ITERATIONS), tv_lambda=0.0 if tv is None else tv,
                       tv_beta=DECONVOLVE_TV_BETA)


def reject_acclimation_conflicts(args):
    """--acclimate_norm's refusals, before anything is built."""
    on = getattr(args, "acclimate_norm", False)
    if not on:
        for flag in ("acclimation_momentum", "acclimation_prior", "acclimation_carry_over"):
            value = getattr(args, flag, None)
            if value is not None and value is not False:
                raise SystemExit("--%s needs --acclimate_norm: it sets how the online batch-norm statistics are averaged and nothing "
                                 "else reads it" % flag)
        return
    if getattr(args, "mode_one_norm", False):
        raise SystemExit("--acclimate_norm with --mode_one_norm: both replace the batch-norm layers' statistics and the layer runs "
                         "one of them (acclimation wins in the reference's layer); choose one")
    if getattr(args, "use_ensemble", False):
        raise SystemExit("--acclimate_norm with --use_ensemble: online statistics are built for a single model; four detectors "
                         "routed per image would each adapt to the part of the stream they are handed")
    if getattr(args, "amp", False):
        raise SystemExit("--amp with --acclimate_norm: the online batch-norm kernel (dib_bn_acclimate_nhwc) and its tolerances are "
                         "fp32; a bf16 lane for it is not built")
    if args.acclimation_prior is not None and args.acclimation_prior < 0:
        raise SystemExit("--acclimation_prior %d: the number of batches the source statistics count for cannot be negative" % args.acclimation_prior)
    m = args.acclimation_momentum
    if m is not None and not (0.0 <= m <= 1.0):
        raise SystemExit("--acclimation_momentum %g: the exponential average's factor lies in [0, 1]" % m)


def _load(model, path):
    if path:
        print("Loading from " + path)
        model.load_state_dict(torch.load(path, map_location="cpu", weights_only=False)["model"])
    return model


def build_deblurer(args, device):
    """reference evaluate.py:240-243: the Deblurer of `--deblur_first` in `--deblur_precision` (never `--amp`'s business), or None"""
    if not getattr(args, "deblur_first", False):
        return None
    from .models.deblur import Deblurer
    return Deblurer(args.deblurer_model_location, device=device, precision=getattr(args, "deblur_precision", "single"))


def main(args):
    from . import kernel_choices
    kernel_choices.use_shipped_kernel_choices()      # shipped MIOpen / TunableOp choices, private copy per process (kernel_choices.py)
    reject_out_of_scope(args)
    reject_acclimation_conflicts(args)
    reject_deconvolution_conflicts(args)
    reject_restoration_metrics_conflicts(args)
    if getattr(args, "deblur_first", False) and not getattr(args, "deblurer_model_location", None):
        raise SystemExit("--deblur_first needs --deblurer_model_location: a DeepDeblur experiment directory (models/model-<N>.pt) or a "
                         "checkpoint file; the reference's default is a path on its author's disk and nothing is downloaded "
                         "(`python -m detectinblur_amd.models.deblur --write_random DIR` writes a random one)")
    mp_ctx = utils.loader_context() if args.workers > 0 else None      # before anything touches the GPU (see utils.loader_context)
    utils.init_distributed_mode(args)
    print(args)
    seed_everything(args.distributed)
    device = torch.device(args.device if torch.cuda.is_available() or args.device == "cpu" else "cpu")
    writer = None
    if utils.is_main_process() and args.tensorboard_path:               # reference evaluate.py:143-151
        from .tb_writer import make_writer
        writer = make_writer(args.tensorboard_path)
    synthetic = dict(num_images=args.synthetic_images, size=tuple(args.synthetic_size), as_tensor=not args.cpu_blur) if args.synthetic else None
    if not (args.gpu_blur or args.cpu_blur or args.vanilla_eval):
        # README: "You'll need to specify --blur_eval and hardware --gpu_blur or --cpu_blur"; without either the
        # reference scores sharp images against the sweep's labels without saying so
        print("Warning: neither --gpu_blur nor --cpu_blur: the sweep will score UNBLURRED images.")

    def detector(path=None, mode_one=False, acclimate=False):
        m = _load(fasterrcnn_resnet50_fpn(num_classes=91, pretrained=args.pretrained, pretrained_backbone=False,
                                          warp_internally=args.warp_in_model, **detector_size_kwargs(args)), path).to(device)
        if mode_one:                                                    # reference evaluate.py:234-237, before DDP wrapping
            from .models.batchnorm import BatchNorm2d
            m = utils.convert_to_custom_batch_norm(m, batch_norm_to_use=BatchNorm2d)
            m = utils.set_batch_norm_N(m, 16)
            m = utils.set_batch_norm_mode1(m, True)
        if acclimate:                                                   # the reference's helpers around its layer's acclimation_mode
            from .models.batchnorm import BatchNorm2d
            prior = ACCLIMATION_PRIOR if args.acclimation_prior is None else args.acclimation_prior
            m = utils.convert_to_custom_batch_norm(m, batch_norm_to_use=BatchNorm2d)
            m = utils.set_batch_norm_N(m, prior)
            if args.acclimation_momentum is None:
                m = utils.set_batch_momentum_zero(m)                    # cumulative: image k of a pass weighs 1 / (prior + k)
            else:
                m = utils.set_batch_momentum(m, args.acclimation_momentum)
            m = utils.set_batch_norm_acclimation_mode(m, True)
            m = utils.copy_BN_stats_to_old(m)                           # what every pass starts from (engine.evaluate restores it)
            m.acclimate_norm = True                                     # engine.evaluate: re-arm the layers after eval()
            m.acclimation_carry_over = bool(args.acclimation_carry_over)
            if args.distributed:
                print("--acclimate_norm: every rank adapts to its own shard of the images (the statistics are not synchronised)")
        if not args.distributed:
            return m
        return torch.nn.parallel.DistributedDataParallel(m, device_ids=[args.gpu] if device.type == "cuda" else None,
                                                         broadcast_buffers=False)

    ensemble, estimator, model = None, None, None
    if args.use_ensemble:                                               # reference evaluate.py:159-205
        if getattr(args, "mode_one_norm", False):
            print("--mode_one_norm is ignored with --use_ensemble (as in the reference: the remedy applies to a single model)")
        # the README passes the four paths as ONE quoted string (evaluate.py:161 splits element 0)
        paths = [q for p_ in (args.ensemble_model_paths or []) for q in p_.split()] or [None] * 4
        ensemble = [detector(p_) for p_ in paths]
        if args.use_blur_estimator or args.blur_estimator_path:
            estimator = resnet18()
            estimator.fc = nn.Linear(512, 4 if args.LEHE else 16)
            estimator = _load(estimator, args.blur_estimator_path).to(device)
    else:
        model = detector(args.resume or args.model_path, mode_one=getattr(args, "mode_one_norm", False),
                         acclimate=getattr(args, "acclimate_norm", False))

    deblurer = build_deblurer(args, device)
    deblur_kw = dict(deblur_first=bool(getattr(args, "deblur_first", False)), deblurer=deblurer)
    deconvolver = build_deconvolver(args)
    deconvolve_kw = dict(deconvolve_first=deconvolver is not None, deconvolver=deconvolver)
    metrics_kw = {}
    if getattr(args, "restoration_metrics", False):      # (off: engine.evaluate is called exactly as before)
        metrics_kw = dict(restoration_metrics=True, restoration_quantize8=bool(getattr(args, "restoration_8bit", False)))

    def loader_for(tf):
        ds, _ = get_coco(args.data_path, "val", tf, synthetic=synthetic, with_masks=getattr(args, "with_masks", False))
        sampler = torch.utils.data.distributed.DistributedSampler(ds) if args.distributed else torch.utils.data.SequentialSampler(ds)
        return torch.utils.data.DataLoader(ds, batch_size=1, sampler=sampler, num_workers=args.workers, collate_fn=utils.collate_fn,
                                           pin_memory=device.type == "cuda", worker_init_fn=_seed_worker, multiprocessing_context=mp_ctx)

    ens_kw = dict(use_ensemble=args.use_ensemble, ensemble_models=ensemble, blur_estimator=estimator, LEHE=args.LEHE)

    def pictures(name):
        """the folder one pass writes its pictures to: None (nothing is written) without --save_images"""
        return os.path.join(args.image_output_dir, name) if getattr(args, "save_images", False) else None
    results = {}
    if args.vanilla_eval:                                               # reference evaluate.py:226-262
        ce = evaluate(model, loader_for(get_transform(False, blur=False)), device=device, vanilla_eval=True,
                      distributed_mode=args.distributed, use_custom_image_norm=args.use_custom_image_norm,
                      early_stop=args.early_stop, image_output_folder=pictures("clean"), **deblur_kw, **ens_kw)
        log_coco_stats(writer, "Clean", ce, 0)
        if writer is not None:
            writer.close()
        return {"Clean": ce}

    # reference evaluate.py:272-370: params[0] / fractions[0] are legacy entries the loops skip, so the tags are
    # P1..P3 over E1..E5
    for param_index, param in enumerate(SWEEP_PARAMS, start=1):
        for fraction_index, fraction in enumerate(SWEEP_FRACTIONS, start=1):
            print("################################## P" + str(param_index) + " and E" + str(fraction_index) + " ###################################")
            tf = get_transform(False, blur=True, blur_type=param, blur_ratio=1, blur_exposure=fraction,
                               use_stored_psfs=args.use_stored_psfs, cpu_blur=args.cpu_blur,
                               stored_psf_directory=args.stored_psf_directory, dont_center_psf=args.dont_center_psf,
                               stored_psf_count=args.stored_psf_count, dilate_psf=args.dilate_psf)
            out = evaluate(model, loader_for(tf), device=device, distributed_mode=args.distributed, early_stop=args.early_stop,
                           blurring_images=True, gpu_blur=args.gpu_blur, expand_target_boxes=args.expand_target_boxes,
                           use_custom_image_norm=args.use_custom_image_norm, add_noise=args.add_noise, noise_level=args.noise_level,
                           add_block=args.add_block, add_jpeg_artifact=args.add_jpeg_artefacts, blur_acc_mode=args.blur_acc_mode,
                           image_output_folder=pictures("P%g_E%g" % (param, fraction)), **deblur_kw, **deconvolve_kw, **ens_kw, **metrics_kw)
            results["P%dE%d" % (param_index, fraction_index - 1)] = out
            if utils.is_main_process():
                log_coco_stats(writer, "P" + str(param_index), out, fraction_index)
            print("P%d E%d: %d images, routes %s" % (param_index, fraction_index - 1, len(out["detections"]), out["routes"][:8]))
            if "restoration" in out:
                from .quality import format_restoration
                res = out["restoration"]
                print("P%d E%d: %s" % (param_index, fraction_index - 1, format_restoration(res)))
                if writer is not None:
                    for name, r in res.items():
                        if isinstance(r, dict):
                            writer.add_scalar("restoration/P%d/%s_psnr_db" % (param_index, name), r["psnr_db"], fraction_index)
                            writer.add_scalar("restoration/P%d/%s_ssim" % (param_index, name), r["ssim"], fraction_index)
                    for gain in ("psnr_gain_db", "ssim_gain"):
                        if gain in res:
                            writer.add_scalar("restoration/P%d/%s" % (param_index, gain), res[gain], fraction_index)
    if writer is not None:
        writer.close()
    return results


if __name__ == "__main__":
    main(build_parser().parse_args())
