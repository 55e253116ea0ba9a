"""`--deblur_first --deblur_precision half` on the GPU: the Half epilogue (dib_bias_act_f16_nhwc) and the Half forms of the three
deblur kernels bit for bit against torch's Half ops on the same device (the pyramid: against the float64 restatement within a derived
bound, and exactly wherever its rounding cannot flip), the whole stage against the torch Half path and the float64 stage, the
engine's hand-over of a Half image, and the driver in a process of its own.  Data and references: tests/test_deblur_half.py."""
import contextlib
import io
import types

import numpy as np
import pytest
import torch

from tests.test_deblur_first import FIXTURE, Recorder, fixture_state, make_image, pyramid_float64, quiet
from tests.test_deblur_first_gpu import DTYPES, SHAPES, evaluate_main_digest_child, float64_stage, odd_image, planar
from tests.test_deblur_half import (EPILOGUE_SHAPES, check_argument_errors_f16, differing_share, epilogue_data, epilogue_want, finish_data,
                                    finish_want)

pytestmark = pytest.mark.gpu

SENTINEL = -777.0                                                # exact in Half


def same_bits(got, want):
    """Half tensors equal bit for bit (-0 is not +0), NaNs at the same places"""
    nan = torch.isnan(want)
    return (got.dtype == want.dtype == torch.float16 and got.shape == want.shape and torch.equal(torch.isnan(got), nan)
            and torch.equal(torch.where(nan, torch.zeros_like(got), got).view(torch.int16), torch.where(nan, torch.zeros_like(want), want).view(torch.int16)))


# ---- dib_bias_act_f16_nhwc --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["bias", "bias_relu", "bias_residual", "bias_residual_relu"])
@pytest.mark.parametrize("chw", EPILOGUE_SHAPES, ids=lambda s: "C%d_%dx%d" % s)
def test_half_epilogue_is_bit_identical(chw, form):
    """C = 8 at 3x5 is 15 lane vectors, less than one block; C = 64 at 9x13 is 936: three blocks and a partial one; C = 3 at 9x13 takes the
    one-element-per-lane kernel (what a coarser scale's 3-channel output gets).  The wrapper launches
    one vector per thread and caps the grid only at 2^30 blocks (csrc/dib_eltwise_vec.h grid_1d: 2^41 elements): no size a test could
    hold takes a second pass of the grid-stride loop."""
    from detectinblur_amd import _lib
    y, b, r = (t.cuda() for t in epilogue_data(*chw))
    double = epilogue_want(y, b, r)
    assert differing_share(double, ((y.float() + b.reshape(1, -1, 1, 1)) + r.float()).half()) >= 0.05      # the data discriminates: first
    res, relu = (r if "residual" in form else None), form.endswith("relu")
    want = epilogue_want(y, b, res, relu)
    got, r_before = y.clone(memory_format=torch.channels_last), r.clone(memory_format=torch.channels_last)
    assert got.is_contiguous(memory_format=torch.channels_last)
    _lib.check(_lib.lib().dib_bias_act_f16_nhwc(got.data_ptr(), b.data_ptr(), res.data_ptr() if res is not None else None, got.numel(), chw[0],
                                                int(relu), _lib.stream_of(got)))
    assert same_bits(got, want) and same_bits(r, r_before)
    # the special values came through as torch leaves them (first pixel: channel k of epilogue_data's rows)
    if chw[0] < 8:
        assert torch.isnan(got[0, 0, 1, 0]) and (form != "bias_residual" or (torch.isnan(got[0, 1, 1, 0]) and got[0, 2, 1, 0] == float("inf")))
        return
    first = got[0, :, 0, 0].float().cpu()
    assert torch.isnan(first[3])
    if form == "bias":
        assert first[0] == 0 and torch.signbit(first[0]) and first[1] == 2.0 ** -24 and first[2] == float("inf") and first[4] == float("inf")
        assert first[5] == 2.0 ** -23 and first[7] == -float("inf")
    if form == "bias_relu":
        assert first[0] == 0 and first[7] == 0 and first[2] == float("inf")           # their sign bits: same_bits above, against torch.relu
    if form == "bias_residual":
        assert first[1] == 2.0 ** -23 and torch.isnan(first[4]) and first[6] == float("inf") and first[5] == 2.0 ** -24
        assert got[0, 6, 0, 1] == -float("inf") and torch.isnan(got[0, 2, 0, 1])


# ---- dib_deblur_pyramid_f16 -------------------------------------------------------------------------------------------------------------

BOUND = 1e-3 + 0.0625 + 0.03125      # the fp32 level's pin + half the Half quantum below 256 + half the quantum of the shifted value


def check_half_pyramid(x, n_scales, levels=None):
    """x: a host image.  Level 0 exact; coarser levels within BOUND of the float64 pyramid minus 127.5; and exactly
    half(half(L) - 127.5) wherever the torch path's fp32 level L on the device cannot round another way within its 1e-3 pin -- at
    least 90 % of every level, which is a condition on the input."""
    from detectinblur_amd.models import deblur as D
    want64 = pyramid_float64(D.quantise(x).numpy(), n_scales)
    got = D.pyramid_device(x.cuda(), n_scales, levels, dtype=torch.float16)
    on_device = D.pyramid(D.pad_to_multiple(D.quantise(x.cuda()), 2 ** (n_scales - 1)), n_scales)
    assert len(got) == n_scales and [g.shape[1] for g in got] == [6] * (n_scales - 1) + [3] and all(g.dtype == torch.float16 for g in got)
    assert np.array_equal(planar(got[0])[:3].astype(np.float64), want64[0] - 127.5)
    for s in range(n_scales):
        g = got[s][0, :3].float()
        assert tuple(g.shape[1:]) == want64[s].shape[1:]
        e64 = float(np.abs(g.cpu().numpy().astype(np.float64) - (want64[s] - 127.5)).max())
        L = on_device[s]
        # level 0 holds integers, computed without a rounding anywhere: every element counts there
        stable = (L - 1e-3).half() == (L + 1e-3).half() if s else torch.ones_like(L, dtype=torch.bool)
        share = float(stable.float().mean())
        exact = (L.half() - 127.5)
        assert exact.dtype == torch.float16
        print(tuple(x.shape), x.dtype, "n", n_scales, "level", s, "vs float64", e64, "stable share", share)
        assert e64 <= (BOUND if s else 0.0) and share >= 0.9
        assert torch.equal(g[stable], exact.float()[stable])
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_half_pyramid_kernel(shape, dtype):
    h, w = shape
    hp, wp = -(-h // 4) * 4, -(-w // 4) * 4
    levels = [torch.full((1, 6 if s < 2 else 3, hp >> s, wp >> s), SENTINEL, device="cuda", dtype=torch.float16).contiguous(memory_format=torch.channels_last)
              for s in range(3)]
    got = check_half_pyramid(odd_image(h, w, dtype), 3, levels)
    for s in range(2):
        assert (got[s][0, 3:] == SENTINEL).all()                              # channels 3..5 are not this kernel's


@pytest.mark.parametrize("n_scales", [1, 2, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
def test_half_pyramid_kernel_at_other_depths(n_scales, dtype):
    """n_scales 1 and 2 need no workspace; 4 chains two fp32 copies"""
    for h, w in ((37, 50), (64, 96), (3, 3)):
        check_half_pyramid(odd_image(h, w, dtype), n_scales)


def test_half_pyramid_kernel_takes_an_unaligned_image():
    from detectinblur_amd.models import deblur as D
    h, w = 64, 96
    x = odd_image(h, w, torch.float16)
    buf = torch.zeros(3 * h * w + 1, dtype=torch.float16, device="cuda")
    shifted = buf[1:].view(3, h, w)
    shifted.copy_(x)
    assert shifted.data_ptr() % 8 != 0
    got = D.pyramid_device(shifted, 3, dtype=torch.float16)
    assert got[0].dtype == torch.float16 and np.array_equal(planar(got[0])[:3].astype(np.float32), D.quantise(x).numpy() - 127.5)


# ---- dib_deblur_shuffle_concat_f16 / dib_deblur_finish_f16 ------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", [(2, 2), (9, 13), (18, 26), (32, 48)], ids=lambda s: "%dx%d" % s)
def test_half_shuffle_concat_kernel_is_bit_identical(hw):
    from detectinblur_amd.models import deblur as D
    h, w = hw
    g = torch.Generator().manual_seed(h * 100 + w)
    cl = torch.channels_last
    raw = (torch.randn(1, 12, h, w, generator=g) * 40).half().cuda().contiguous(memory_format=cl)
    bias = torch.randn(12, generator=g).half().float().cuda()
    level = torch.randn(1, 6, 2 * h, 2 * w, generator=g).half().cuda().contiguous(memory_format=cl)
    before = level.clone(memory_format=cl)
    want = torch.cat((level[:, :3], torch.nn.functional.pixel_shuffle(raw + bias.half().reshape(1, -1, 1, 1), 2)), 1)
    assert want.dtype == torch.float16
    got = D.shuffle_concat_device(raw, bias, level)
    assert got is level and same_bits(got, want) and torch.equal(got[:, :3], before[:, :3])      # channels 0..2 are untouched
    assert differing_share(got[:, 3:].contiguous(), before[:, 3:].contiguous()) > 0.9


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_half_finish_kernel_is_bit_identical(shape):
    from detectinblur_amd.models import deblur as D
    h, w = shape
    raw, bias = (t.cuda() for t in finish_data(h, w))
    want = finish_want(raw, bias, h, w)
    x = raw.float()[0, :, :h, :w] + bias.reshape(-1, 1, 1)
    single = (((x + 127.5) + 0.5).clamp(0, 255) * (1.0 / 255.0)).half()
    assert differing_share(want, single) >= 0.02                            # the data discriminates: first
    got = D.finish_device(raw.contiguous(memory_format=torch.channels_last), bias, h, w)
    assert got.dtype == torch.float16 and tuple(got.shape) == (3, h, w) and got.is_contiguous()
    nan = torch.isnan(want)
    assert bool(nan[1, 0, 0]) and int(nan.sum()) == 1 and same_bits(got, want)
    assert float(got[2, h - 1, w - 1]) == 1.0 and float(got[0, h // 2, w // 2]) == 0.0 and float(got[0, 0, 1]) == 0.0 and float(got[1, 0, 1]) == 1.0
    assert 0.2 < float(((got > 0) & (got < 1)).float().mean()) < 0.8


def test_argument_errors_return_einval_without_a_launch():
    check_argument_errors_f16()
    torch.cuda.synchronize()


# ---- the whole stage --------------------------------------------------------------------------------------------------------------------

def half_stage_errors(location, x):
    from detectinblur_amd.models import deblur as D
    want = float64_stage(quiet(D.Deblurer, location), x)
    d = quiet(D.Deblurer, location, torch.device("cuda", 0), precision="half")
    assert d.model.n_feats % 8 == 0 and all(p.dtype == torch.float16 for p in d.parameters())
    hip = d.deblur_(x.cuda())
    assert d.last_path == "hip" and hip.dtype == torch.float16 and hip.is_cuda and tuple(hip.shape) == tuple(x.shape)
    D.FUSE_DEBLUR = False
    try:
        plain = d.deblur_(x.cuda())
        assert d.last_path == "torch" and plain.dtype == torch.float16
    finally:
        D.FUSE_DEBLUR = True
    inside = float(((want > 0.02) & (want < 0.98)).mean())
    e_hip, e_torch = float(np.abs(hip.float().cpu().numpy() - want).max()), float(np.abs(plain.float().cpu().numpy() - want).max())
    e_between = float((hip.float() - plain.float()).abs().max())
    return e_hip, e_torch, e_between, inside


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
def test_whole_half_stage_with_the_fixtures_network(tmp_path, dtype):
    """the tiny net of tests/golden/deblur_pins.npz at 37x50.  Bound: twice the error of the plain torch Half path on the same device
    against float64 (the HIP path calls MIOpen without a bias, which may pick another solver; every other op is the same Half op).
    Measured on an MI355X: profiles/deblur_half.txt."""
    with np.load(FIXTURE) as f:
        state = fixture_state({k: f[k] for k in f.files})
    path = str(tmp_path / "fixture.pt")
    torch.save({"G": state}, path)
    e_hip, e_torch, e_between, inside = half_stage_errors(path, make_image(37, 50, dtype))
    print("tiny net", dtype, "half: HIP vs float64", e_hip, "torch GPU vs float64", e_torch, "HIP vs torch GPU", e_between, "unsaturated", inside)
    assert inside > 0.5 and e_torch > 0 and e_hip <= 2 * e_torch


def test_whole_half_stage_at_the_real_widths(tmp_path):
    """n_feats 64, n_resblocks 19, k 5, three scales, seeded by write_random_checkpoint, on a 36x52 image: same bound"""
    from detectinblur_amd.models.deblur import write_random_checkpoint
    write_random_checkpoint(str(tmp_path), seed=0)
    e_hip, e_torch, e_between, inside = half_stage_errors(str(tmp_path), make_image(36, 52, torch.float16))
    print("real widths, half: HIP vs float64", e_hip, "torch GPU vs float64", e_torch, "HIP vs torch GPU", e_between, "unsaturated", inside)
    assert inside > 0.5 and e_torch > 0 and e_hip <= 2 * e_torch


# ---- engine.evaluate ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pipelined", [False, True], ids=["plain", "pipelined"])
def test_engine_hands_the_detector_and_the_overlay_the_half_image(tmp_path, monkeypatch, pipelined):
    """tests/test_deblur_first_gpu.py's hand-over test with a precision="half" deblurrer and a detector whose input transform is the
    fused one (as the real detector's is: engine._to_float then leaves Half images alone): the detector and the picture get exactly
    Deblurer.deblur_ of the blurred Half image, in Half, and the loop synchronises no more often than without the stage"""
    import random
    from detectinblur_amd import engine, overlay
    from detectinblur_amd.models.deblur import Deblurer, write_random_checkpoint
    from tests.test_overlay import fixed_detections, read_png, synthetic_loader
    from tests.test_overlay_gpu import SplitDetector
    if pipelined:
        monkeypatch.delenv("DIB_NO_PIPELINE", raising=False)
    else:
        monkeypatch.setenv("DIB_NO_PIPELINE", "1")
    monkeypatch.delenv("DIB_NO_GRAPHS", raising=False)
    h, w, n = 70, 101, 3
    write_random_checkpoint(str(tmp_path / "ck"), n_feats=8, n_resblocks=2, seed=3)
    device = torch.device("cuda", 0)
    real = quiet(Deblurer, str(tmp_path / "ck"), device, precision="half")
    dets = fixed_detections(h, w)
    np.random.seed(11)
    random.seed(11)
    loader = synthetic_loader(h, w, n=n, blur=True, blur_type=0.001, blur_ratio=1, blur_exposure=0.5)
    syncs = [0]
    real_sync = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: syncs.__setitem__(0, syncs[0] + 1) or real_sync(*a, **k))

    def run(folder=None, **kw):
        model = SplitDetector(dets)
        model.transform = types.SimpleNamespace(fused=True)
        syncs[0] = 0
        with contextlib.redirect_stdout(io.StringIO()):
            engine.evaluate(None, loader, device, blurring_images=True, gpu_blur=True, expand_target_boxes=True, use_ensemble=True,
                            ensemble_models=[model] * 4, image_output_folder=folder, **kw)
        return model.seen, syncs[0]
    blurred, syncs_plain = run()
    spy = Recorder(real)
    seen, syncs_deblur = run(folder=str(tmp_path / "pics"), deblur_first=True, deblurer=spy)
    assert syncs_deblur == syncs_plain and len(seen) == n and len(spy.inputs) == n
    for i in range(n):
        assert blurred[i].dtype == torch.float16 and spy.inputs[i].dtype == torch.float16 and torch.equal(spy.inputs[i], blurred[i])
        assert seen[i].dtype == torch.float16 and seen[i].is_cuda and torch.equal(seen[i], spy.outputs[i])
        assert torch.equal(seen[i], real.deblur_(spy.inputs[i])) and real.last_path == "hip"
        assert not torch.equal(seen[i], blurred[i])
        want = overlay.render_host(seen[i].cpu(), dets[i]["boxes"], dets[i]["labels"], dets[i]["scores"])
        assert np.array_equal(read_png(tmp_path / "pics" / ("img%d.png" % i)), want), i


# ---- the driver, in a process of its own -------------------------------------------------------------------------------------------------

def test_evaluate_main_runs_the_sweep_in_half(tmp_path):
    """No run-to-run identity is asserted: MIOpen ranks its Half solvers by a search of its own in every process (no shipped records)."""
    from detectinblur_amd.models.deblur import write_random_checkpoint
    from tests.test_ddp_gpu import _run_child
    write_random_checkpoint(str(tmp_path / "ck"), n_feats=8, n_resblocks=2, seed=3)
    argv = ["--synthetic", "--synthetic_images", "3", "--synthetic_size", "128", "160", "--min_size", "128", "--max_size", "160", "--blur_eval",
            "--gpu_blur", "--expand_target_boxes", "--early_stop", "2", "--deblur_first", "--deblur_precision", "half",
            "--deblurer_model_location", str(tmp_path / "ck"), "--tensorboard_path", str(tmp_path / "tb")]
    (tmp_path / "a").mkdir()
    a = _run_child(evaluate_main_digest_child, tmp_path / "a", argv, timeout=600)
    assert len(a["cells"]) == 15 and len(a["stat_lines"]) == 12 * 15
    for cell in a["cells"]:
        stats = a["cells"][cell]["stats"]
        assert a["cells"][cell]["images"] == 3 and len(stats) == 12 and all(np.isfinite(v) for v in stats), cell
