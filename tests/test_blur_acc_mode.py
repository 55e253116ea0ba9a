"""`--blur_acc_mode {bitexact,fp32,fma16,fast16}` without a GPU: the three parsers, the refusal of a mode that no launch would run,
the resolver that decides what a mode means for a batch (blur_ops.resolve_acc_mode: the whole table), and the flag's way down
from the three `main()` functions to `models.blur_functions.blur_image_list` (replaced by a recorder: nothing is blurred)."""
import contextlib
import inspect
import io

import pytest
import torch

from detectinblur_amd import _lib, blur_ops

MODES = {"bitexact": _lib.DIB_ACC_BITEXACT, "fp32": _lib.DIB_ACC_FP32, "fma16": _lib.DIB_ACC_FMA16, "fast16": _lib.DIB_ACC_FAST16}


def _parsers():
    from detectinblur_amd import evaluate, train, train_blur_estimator
    return {"train": train, "evaluate": evaluate, "train_blur_estimator": train_blur_estimator}


# ---- parsers ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("driver", ["train", "evaluate", "train_blur_estimator"])
def test_every_parser_takes_the_flag(driver, capsys):
    p = _parsers()[driver].build_parser()
    assert p.parse_args([]).blur_acc_mode == "bitexact"
    for mode in MODES:
        assert p.parse_args(["--gpu_blur", "--blur_acc_mode", mode]).blur_acc_mode == mode
    with pytest.raises(SystemExit) as e:
        p.parse_args(["--blur_acc_mode", "fp64"])
    assert e.value.code == 2 and "invalid choice" in capsys.readouterr().err
    text = " ".join(p.format_help().split())
    assert "--blur_acc_mode" in text and "(this repo)" in text
    for stated in ("5e-3", "1e-2"):
        assert stated in text


def test_the_names_are_the_library_constants():
    from detectinblur_amd import train
    assert blur_ops.ACC_MODES == MODES and tuple(blur_ops.ACC_MODES) == train.BLUR_ACC_MODES
    assert blur_ops.ACC_MODE_TOLERANCE == {"bitexact": 0.0, "fp32": 5e-3, "fma16": 1e-2, "fast16": 1e-2}


@pytest.mark.parametrize("driver", ["train", "evaluate", "train_blur_estimator"])
@pytest.mark.parametrize("mode", ["fp32", "fma16", "fast16"])
def test_a_mode_that_nothing_would_run_is_refused_at_start(driver, mode):
    """Without --gpu_blur, or with --cpu_blur (the detector drivers have that flag), a tolerance mode would silently do nothing:
    `main` stops with a SystemExit that names both flags, before it builds anything."""
    mod = _parsers()[driver]
    base = ["--synthetic", "--device", "cpu", "--blur_acc_mode", mode]
    with pytest.raises(SystemExit) as e, contextlib.redirect_stdout(io.StringIO()):
        mod.main(mod.build_parser().parse_args(base))
    assert "--blur_acc_mode" in str(e.value) and "--gpu_blur" in str(e.value)
    if driver != "train_blur_estimator":
        for extra in (["--cpu_blur"], ["--cpu_blur", "--gpu_blur"]):
            with pytest.raises(SystemExit) as e, contextlib.redirect_stdout(io.StringIO()):
                mod.main(mod.build_parser().parse_args(base + extra))
            assert "--blur_acc_mode" in str(e.value) and "--cpu_blur" in str(e.value)


def test_the_default_and_a_served_mode_pass_the_check():
    from detectinblur_amd import train
    p = train.build_parser()
    train.reject_out_of_scope(p.parse_args(["--synthetic"]))
    train.reject_out_of_scope(p.parse_args(["--synthetic", "--cpu_blur"]))
    train.reject_out_of_scope(p.parse_args(["--synthetic", "--cpu_blur", "--blur_acc_mode", "bitexact"]))
    train.reject_out_of_scope(p.parse_args(["--synthetic", "--gpu_blur", "--blur_acc_mode", "fast16"]))


# ---- resolver: the whole table -------------------------------------------------------------------------------------
# (mode, K, large window wanted) -> (constant, vruns, large window) on fp16 images
F16 = [
    ("bitexact", 128, False, ("bitexact", False, False)), ("bitexact", 128, True, ("bitexact", False, True)),
    ("bitexact", 256, False, ("bitexact", False, False)), ("bitexact", 256, True, ("bitexact", False, True)),
    ("fma16", 128, False, ("fma16", False, False)), ("fma16", 128, True, ("fma16", False, True)),
    ("fma16", 256, False, ("fma16", False, False)), ("fma16", 256, True, ("fma16", False, True)),
    # fp32 and fast16 always take the standard window
    ("fp32", 128, False, ("fp32", False, False)), ("fp32", 128, True, ("fp32", False, False)),
    ("fp32", 256, False, ("fp32", False, False)), ("fp32", 256, True, ("fp32", False, False)),      # K = 256 with fp32 is served
    ("fast16", 128, False, ("fast16", True, False)), ("fast16", 128, True, ("fast16", True, False)),
    # K = 256 with fast16: fma16 (row-major order, the same arithmetic class); the window is then fma16's to take
    ("fast16", 256, False, ("fma16", False, False)), ("fast16", 256, True, ("fma16", False, True)),
]


@pytest.mark.parametrize("mode,K,large,want", F16, ids=["%s-K%d-%s" % (m, k, "large" if l else "std") for m, k, l, _ in F16])
def test_resolver_on_fp16_images(mode, K, large, want):
    exp = (MODES[want[0]], want[1], want[2])
    assert blur_ops.resolve_acc_mode(mode, K, torch.float16, large) == exp            # by name
    assert blur_ops.resolve_acc_mode(MODES[mode], K, torch.float16, large) == exp     # by constant
    got = blur_ops.resolve_acc_mode(mode, K, torch.float16, large)
    assert type(got[1]) is bool and type(got[2]) is bool


@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("large", [False, True])
def test_resolver_on_fp32_images(K, large):
    """fp32 images already accumulate in fp32: the default passes (standard window: the large one serves fp16 tiles only), every
    other mode is a ValueError -- and the library's own error type, which manual_blur's callers were promised before."""
    assert blur_ops.resolve_acc_mode("bitexact", K, torch.float32, large) == (_lib.DIB_ACC_BITEXACT, False, False)
    for mode in ("fp32", "fma16", "fast16"):
        for m in (mode, MODES[mode]):
            with pytest.raises(ValueError, match="fp16 images only") as e:
                blur_ops.resolve_acc_mode(m, K, torch.float32, large)
            assert isinstance(e.value, _lib.DibError)


def test_resolver_refuses_what_it_does_not_know_and_can_be_told_not_to_substitute():
    for bad in ("fp64", "FAST16", 4, -1, None):
        with pytest.raises(ValueError, match="unknown blur accumulation mode"):
            blur_ops.resolve_acc_mode(bad, 128, torch.float16)
    # manual_blur names the very arithmetic it wants: no other mode in its place
    with pytest.raises(ValueError, match="128 canvas"):
        blur_ops.resolve_acc_mode("fast16", 256, torch.float16, substitute=False)
    assert blur_ops.resolve_acc_mode("fast16", 128, torch.float16, substitute=False) == (_lib.DIB_ACC_FAST16, True, False)


# ---- reach: the flag arrives at the blur call of every driver -----------------------------------------------------------

@pytest.fixture
def recorder(monkeypatch):
    """models.blur_functions.blur_image_list replaced by a function that notes the `acc_mode` of every call and blurs nothing."""
    from detectinblur_amd.models import blur_functions as BF
    sig = inspect.signature(BF.blur_image_list)
    seen = []

    def record(*a, **k):
        seen.append(sig.bind(*a, **k).arguments.get("acc_mode", sig.parameters["acc_mode"].default))
        return None
    monkeypatch.setattr(BF, "blur_image_list", record)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    return seen


def _quiet(fn, *a):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a)


_SMALL = ["--synthetic", "--synthetic_images", "2", "--synthetic_size", "96", "128", "--device", "cpu", "--gpu_blur"]


@pytest.mark.parametrize("flag,want", [(["--blur_acc_mode", "fast16"], _lib.DIB_ACC_FAST16), ([], _lib.DIB_ACC_BITEXACT)], ids=["fast16", "absent"])
def test_train_main_hands_the_mode_to_every_blur_call(recorder, monkeypatch, flag, want):
    import detectinblur_amd.train as TR
    from tests.test_engine_ddp_cpu import _small_model
    monkeypatch.setattr(TR, "fasterrcnn_resnet50_fpn", lambda **kw: _small_model())
    argv = _SMALL + ["--blur_train", "-b", "2", "--epochs", "1", "--early_stop", "0", "--lr", "0.001", "--print_freq", "1", "--output_dir", "",
                     "--tensorboard_path", ""] + flag
    _quiet(TR.main, TR.build_parser().parse_args(argv))
    assert len(recorder) >= 2 and all(m == want for m in recorder), recorder      # the training step AND the blurred evaluation


class _FirstCell(Exception):
    pass


@pytest.mark.parametrize("flag,want", [(["--blur_acc_mode", "fast16"], _lib.DIB_ACC_FAST16), ([], _lib.DIB_ACC_BITEXACT)], ids=["fast16", "absent"])
def test_evaluate_main_hands_the_mode_to_every_blur_call(recorder, monkeypatch, flag, want):
    import detectinblur_amd.evaluate as EV
    from tests.test_engine_ddp_cpu import _small_model
    monkeypatch.setattr(EV, "fasterrcnn_resnet50_fpn", lambda **kw: _small_model())
    real = EV.evaluate

    def first_cell(*a, **k):          # the sweep's first cell is all this needs
        real(*a, **k)
        raise _FirstCell()
    monkeypatch.setattr(EV, "evaluate", first_cell)
    argv = _SMALL + ["--blur_eval", "--early_stop", "1", "--tensorboard_path", ""] + flag
    with pytest.raises(_FirstCell):
        _quiet(EV.main, EV.build_parser().parse_args(argv))
    assert len(recorder) >= 2 and all(m == want for m in recorder), recorder


@pytest.mark.parametrize("flag,want", [(["--blur_acc_mode", "fast16"], _lib.DIB_ACC_FAST16), ([], _lib.DIB_ACC_BITEXACT)], ids=["fast16", "absent"])
@pytest.mark.parametrize("resize", [False, True], ids=["plain", "resize_images"])
def test_estimator_main_hands_the_mode_to_every_blur_call(recorder, flag, want, resize):
    import detectinblur_amd.train_blur_estimator as TB
    # (--LEHE_blur_seg: the evaluation's per-class summary looks at labels 0..3, as the reference's does)
    argv = _SMALL + ["--blur_train", "--LEHE_blur_seg", "-b", "2", "--epochs", "1", "--early_stop", "0", "--lr", "0.001", "--output_dir", ""] + flag
    if resize:
        argv = argv + ["--resize_images"]
    _quiet(TB.main, TB.build_parser().parse_args(argv))
    assert len(recorder) >= 2 and all(m == want for m in recorder), recorder      # the training step AND the evaluation
