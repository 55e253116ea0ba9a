"""`--deblur_first` on the GPU: the three kernels of csrc/dib_deblur.hip against the torch path on the same device and against the
float64 restatement of tests/test_deblur_first.py, the whole stage (HIP kernels + MIOpen convolutions + dib_bias_act_nhwc) against a
float64 CPU run of the same module, the engine's hand-over inside the pipelined loop, and the driver in fresh processes."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

from tests.test_deblur_first import (FIXTURE, Recorder, check_argument_errors, every_half_in_unit_interval, fixture_state, make_image,
                                     pyramid_float64, quiet)

pytestmark = pytest.mark.gpu

# 70x101 pads to 72x104: levels 36x52 and 18x26 cross the 16-pixel output tiles of the down kernel in both directions (3 x 4 and 2 x 2
# workgroups, the last ones partial); 5x6 pads to 8x8 with a 2x2 coarsest level (halo longer than the image); 64x96 is the aligned case
SHAPES = [(5, 6), (37, 50), (70, 101), (64, 96)]
DTYPES = [torch.float16, torch.float32]


def odd_image(h, w, dtype):
    """seeded [0, 1] values with a few outside the reference's domain (this library's choice there: clamp, NaN -> 0)"""
    x = make_image(h, w, torch.float32)
    flat = x.reshape(-1)
    odd = torch.tensor([float("nan"), -0.5, 2.0, float("inf"), 1.0, 0.0, 0.50195312])
    n = min(odd.numel(), flat.numel())
    flat[torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(h))[:n]] = odd[:n]
    return x.to(dtype)


def planar(level):
    """a channels-last [1, C, h, w] level -> [C, h, w] on the host"""
    return level[0].cpu().contiguous().numpy()


# ---- dib_deblur_pyramid ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_pyramid_kernel(shape, dtype):
    from detectinblur_amd.models import deblur as D
    h, w = shape
    x = odd_image(h, w, dtype)
    q = D.quantise(x)
    want64 = pyramid_float64(q.numpy())
    hp, wp = want64[0].shape[1:]
    levels = [torch.full((1, 6 if s < 2 else 3, hp >> s, wp >> s), -777.0, device="cuda").contiguous(memory_format=torch.channels_last) for s in range(3)]
    got = D.pyramid_device(x.cuda(), 3, levels)
    on_device = D.pyramid(D.pad_to_multiple(D.quantise(x.cuda()), 4), 3)                 # the torch path on the same device
    assert np.array_equal(planar(got[0])[:3], want64[0] - 127.5)                          # the integer level: exact
    for s in range(3):
        g = planar(got[s])
        e64 = float(np.abs(g[:3] - (want64[s] - 127.5)).max())
        et = float(np.abs(g[:3] - (on_device[s].cpu().numpy() - 127.5)).max())
        print(shape, dtype, "level", s, "vs float64", e64, "vs torch path", et)
        assert g.shape[1:] == want64[s].shape[1:] and e64 <= 1e-3 and et <= 1e-3
        assert s == 2 or (g[3:] == -777.0).all()                                          # channels 3..5 are not this kernel's


@pytest.mark.parametrize("n_scales", [1, 2, 4])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
def test_pyramid_kernel_at_other_depths(n_scales, dtype):
    """n_scales 1: only the 3-channel level (16-byte stores at 64x96, element stores at 37x50); 2: padded widths that are no multiple of 4"""
    from detectinblur_amd.models import deblur as D
    for h, w in ((37, 50), (64, 96), (3, 3)):
        x = odd_image(h, w, dtype)
        want64 = pyramid_float64(D.quantise(x).numpy(), n_scales)
        got = D.pyramid_device(x.cuda(), n_scales)
        assert len(got) == n_scales and [g.shape[1] for g in got] == [6] * (n_scales - 1) + [3]
        assert np.array_equal(planar(got[0])[:3], want64[0] - 127.5)
        for s in range(n_scales):
            assert float(np.abs(planar(got[s])[:3] - (want64[s] - 127.5)).max()) <= 1e-3, (h, w, s)


def test_pyramid_kernel_takes_an_unaligned_image():
    from detectinblur_amd.models import deblur as D
    h, w = 64, 96
    x = odd_image(h, w, torch.float16)
    buf = torch.zeros(3 * h * w + 1, dtype=torch.float16, device="cuda")
    shifted = buf[1:].view(3, h, w)
    shifted.copy_(x)
    assert shifted.data_ptr() % 8 != 0
    assert np.array_equal(planar(D.pyramid_device(shifted, 3)[0])[:3], D.quantise(x).numpy() - 127.5)


def test_every_half_value_is_quantised_exactly():
    from detectinblur_amd.models import deblur as D
    x = every_half_in_unit_interval()
    want = np.trunc((x.numpy() * np.float16(255)).astype(np.float16).astype(np.float32))
    got = planar(D.pyramid_device(x.cuda(), 1)[0])
    assert got.shape == want.shape and np.array_equal(got, want - 127.5)
    assert 128 in want and np.array_equal(planar(D.pyramid_device(x.float().cuda(), 1)[0]), np.trunc(x.float().numpy() * np.float32(255)) - 127.5)


# ---- dib_deblur_shuffle_concat / dib_deblur_finish ------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", [(2, 2), (9, 13), (18, 26), (32, 48)], ids=lambda s: "%dx%d" % s)
def test_shuffle_concat_kernel_is_bit_identical(hw):
    from detectinblur_amd.models import deblur as D
    h, w = hw
    g = torch.Generator().manual_seed(h * 100 + w)
    raw = (torch.randn(1, 12, h, w, generator=g) * 40).cuda().contiguous(memory_format=torch.channels_last)
    bias = torch.randn(12, generator=g).cuda()
    level = torch.randn(1, 6, 2 * h, 2 * w, generator=g).cuda().contiguous(memory_format=torch.channels_last)
    want = torch.cat((level[:, :3], torch.nn.functional.pixel_shuffle(raw + bias.reshape(1, -1, 1, 1), 2)), 1)
    got = D.shuffle_concat_device(raw, bias, level)
    assert got is level and torch.equal(got, want)


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_finish_kernel_is_bit_identical(shape):
    from detectinblur_amd.models import deblur as D
    h, w = shape
    hp, wp = -(-h // 4) * 4, -(-w // 4) * 4
    g = torch.Generator().manual_seed(h * 1000 + w)
    raw = torch.rand(1, 3, hp, wp, generator=g) * 600 - 300                 # v + 127.5 straddles 0 and 255
    raw[0, 1, 0, 0], raw[0, 2, h - 1, w - 1], raw[0, 0, h // 2, w // 2] = float("nan"), float("inf"), -float("inf")
    raw[0, 0, 0, 1], raw[0, 1, 0, 1] = -128.0, 127.0                        # lands on the clamp's ends exactly (bias 0 below)
    raw = raw.cuda().contiguous(memory_format=torch.channels_last)
    bias = torch.tensor([0.0, 0.3, -7.25], device="cuda")
    want = ((raw + bias.reshape(1, -1, 1, 1)) + 127.5)[0, :, :h, :w].clone().add_(0.5).clamp_(0, 255) / 255
    got = D.finish_device(raw, bias, h, w)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, h, w) and got.is_contiguous()
    nan = torch.isnan(want)
    assert bool(nan[1, 0, 0]) and int(nan.sum()) == 1 and torch.equal(torch.isnan(got), nan)       # the NaN comes out as torch leaves it
    assert torch.equal(torch.where(nan, torch.zeros_like(got), got), torch.where(nan, torch.zeros_like(want), want))
    assert float(got[2, h - 1, w - 1]) == 1.0 and float(got[0, h // 2, w // 2]) == 0.0 and float(got[0, 0, 1]) == 0.0 and float(got[1, 0, 1]) == 1.0
    assert 0.2 < float(((got > 0) & (got < 1)).float().mean()) < 0.8


def test_argument_errors_return_einval_without_a_launch():
    check_argument_errors()
    torch.cuda.synchronize()


# ---- the whole stage --------------------------------------------------------------------------------------------------------------------

def float64_stage(deblurrer_cpu, x):
    """steps 1-5 in float64 on the host: scipy's pyramid, the same module's weights as doubles"""
    import copy
    from detectinblur_amd.models import deblur as D
    h, w = x.shape[1:]
    net = copy.deepcopy(deblurrer_cpu.model).double()
    levels = pyramid_float64(D.quantise(x).numpy(), net.n_scales)
    with torch.no_grad():
        out = net([torch.from_numpy(l)[None] for l in levels])[0]
    return ((out[0, :, :h, :w] + 0.5).clamp(0, 255) / 255).numpy()


def stage_errors(location, x):
    from detectinblur_amd.models import deblur as D
    want = float64_stage(quiet(D.Deblurer, location), x)
    d = quiet(D.Deblurer, location, torch.device("cuda", 0))
    assert d.model.n_feats % 4 == 0
    hip = d.deblur_(x.cuda())
    assert d.last_path == "hip" and hip.dtype == torch.float32 and hip.is_cuda and tuple(hip.shape) == tuple(x.shape)
    D.FUSE_DEBLUR = False
    try:
        plain = d.deblur_(x.cuda())
        assert d.last_path == "torch"
    finally:
        D.FUSE_DEBLUR = True
    inside = float(((want > 0.02) & (want < 0.98)).mean())
    e_hip, e_torch = float(np.abs(hip.cpu().numpy() - want).max()), float(np.abs(plain.cpu().numpy() - want).max())
    return e_hip, e_torch, inside


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "f32"])
def test_whole_stage_with_the_fixtures_network(tmp_path, dtype):
    """the tiny net of tests/golden/deblur_pins.npz (n_feats 8, 2 blocks) at 37x50.  Bound: twice the error of the plain-torch GPU path
    (MIOpen with the bias inside) against float64 -- the HIP path adds the bias and the residual in another order, nothing else.
    Measured on an MI355X (scale 0..1): f16 4.23e-7 against 4.23e-7, f32 3.83e-7 against 3.38e-7 (profiles/deblur_first.txt)."""
    with np.load(FIXTURE) as f:
        state = fixture_state({k: f[k] for k in f.files})
    path = str(tmp_path / "fixture.pt")
    torch.save({"G": state}, path)
    e_hip, e_torch, inside = stage_errors(path, make_image(37, 50, dtype))
    print("tiny net", dtype, "HIP vs float64", e_hip, "torch GPU vs float64", e_torch, "unsaturated", inside)
    assert inside > 0.5 and e_torch > 0 and e_hip <= 2 * e_torch


def test_whole_stage_at_the_real_widths(tmp_path):
    """n_feats 64, n_resblocks 19, k 5, three scales, seeded by write_random_checkpoint, on a 36x52 image: same bound.
    Measured on an MI355X: 3.74e-7 against 4.00e-7."""
    from detectinblur_amd.models.deblur import write_random_checkpoint
    write_random_checkpoint(str(tmp_path), seed=0)
    e_hip, e_torch, inside = stage_errors(str(tmp_path), make_image(36, 52, torch.float16))
    print("real widths: HIP vs float64", e_hip, "torch GPU vs float64", e_torch, "unsaturated", inside)
    assert inside > 0.5 and e_torch > 0 and e_hip <= 2 * e_torch


# ---- engine.evaluate ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pipelined", [False, True], ids=["plain", "pipelined"])
def test_engine_hands_the_detector_and_the_overlay_the_deblurred_image(tmp_path, monkeypatch, pipelined):
    """after --gpu_blur and the box growth, in the look-ahead: the detector and the picture get Deblurer.deblur_ of the blurred Half image,
    fp32, through the HIP path, and the loop synchronises no more often than without the stage"""
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
    real = quiet(Deblurer, str(tmp_path / "ck"), device)
    dets = fixed_detections(h, w)
    np.random.seed(11)
    random.seed(11)
    loader = synthetic_loader(h, w, n=n, blur=True, blur_type=0.001, blur_ratio=1, blur_exposure=0.5)
    syncs = [0]
    real_sync = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: syncs.__setitem__(0, syncs[0] + 1) or real_sync(*a, **k))

    def run(folder=None, **kw):
        model = SplitDetector(dets)
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
        assert spy.inputs[i].dtype == torch.float16 and torch.equal(spy.inputs[i].float(), blurred[i])      # the blurred image
        assert seen[i].dtype == torch.float32 and seen[i].is_cuda and torch.equal(seen[i], spy.outputs[i])
        assert torch.equal(seen[i], real.deblur_(spy.inputs[i])) and real.last_path == "hip"
        want = overlay.render_host(seen[i].cpu(), dets[i]["boxes"], dets[i]["labels"], dets[i]["scores"])
        assert np.array_equal(read_png(tmp_path / "pics" / ("img%d.png" % i)), want), i


# ---- the driver, in processes of its own ---------------------------------------------------------------------------------------------

def evaluate_main_digest_child(out_path, argv):
    from tests import _gpu_children
    _gpu_children._guarded(_gpu_children._evaluate_main_digest, out_path, (argv,))


def test_two_runs_of_evaluate_main_print_identical_coco_stats_and_a_third_writes_pictures(tmp_path):
    from detectinblur_amd.models.deblur import write_random_checkpoint
    from tests.test_ddp_gpu import _run_child
    write_random_checkpoint(str(tmp_path / "ck"), n_feats=8, n_resblocks=2, seed=3)
    argv = ["--synthetic", "--synthetic_images", "3", "--synthetic_size", "128", "160", "--min_size", "128", "--max_size", "160", "--blur_eval",
            "--gpu_blur", "--expand_target_boxes", "--early_stop", "2", "--deblur_first", "--deblurer_model_location", str(tmp_path / "ck"),
            "--tensorboard_path", str(tmp_path / "tb")]
    for name in "abc":
        (tmp_path / name).mkdir()
    a = _run_child(evaluate_main_digest_child, tmp_path / "a", argv, timeout=600)
    b = _run_child(evaluate_main_digest_child, tmp_path / "b", argv, timeout=600)
    assert len(a["stat_lines"]) == 12 * 15 and a["stat_lines"] == b["stat_lines"]
    for cell in a["cells"]:
        assert a["cells"][cell]["images"] == 3 and a["cells"][cell]["stats"] == b["cells"][cell]["stats"], cell
    pics = tmp_path / "pics"
    c = _run_child(evaluate_main_digest_child, tmp_path / "c", argv + ["--save_images", "--image_output_dir", str(pics)], timeout=600)
    assert c["stat_lines"] == a["stat_lines"]
    folders = sorted(os.listdir(pics))
    assert len(folders) == 15 and all(sorted(os.listdir(pics / f)) == ["img0.png", "img1.png", "img2.png"] for f in folders)
