"""The DeepDeblur trainer's mixed-precision step (--amp) without a GPU: the Half forms of the torch restatements against float64, the
summation depth with 8 channels per lane against counts made by hand, and the driver end to end on the CPU, where the network takes the
autocast path ("torch-amp"): the scaler's plumbing, the checkpoint layout, --resume, the refusals, and steps skipped on an overflow."""
import contextlib
import io
import re

import pytest
import torch

from detectinblur_amd import train_deblurrer as TD
from detectinblur_amd.models import deblur
from detectinblur_amd.models import deblur_train as DT
from tests.test_deblur_train import TINY


# ---- restatements against float64 -------------------------------------------------------------------------------------------------

def test_half_mask_layout_is_one_byte_per_eight_elements():
    y = torch.zeros(3, 16, dtype=torch.float16)
    y[0, 0], y[0, 7], y[1, 9], y[2, 15] = 1.0, 6e-8, 2.0, float("inf")         # 6e-8: Half's smallest denormal, > 0
    y[0, 1], y[0, 2], y[1, 10] = float("nan"), -0.0, -1.0                      # no bit: a NaN, a zero, a negative
    mask = DT.sign_mask_torch(y)
    assert mask.dtype == torch.uint8 and mask.numel() == 3 * 16 // 8
    assert mask.tolist() == [0x81, 0, 0, 0x02, 0, 0x80]
    # the fp32 layout is untouched: one byte per 4
    assert DT.sign_mask_torch(y.float()).tolist() == [1, 8, 0, 0, 0, 0, 2, 0, 0, 0, 0, 8]


def test_half_bias_grad_restatement_against_float64():
    g = torch.Generator().manual_seed(1)
    n_pix, C = 37, 16
    y = torch.randn(n_pix, C, generator=g).half()
    y[3, 2], y[4, 1] = float("nan"), 0.0
    grad = (torch.randn(n_pix, C, generator=g) * 300).half()
    grad[5, 3], grad[6, 6] = float("nan"), float("inf")
    y[5, 3], y[6, 6] = 1.0, 2.0                     # both pass the mask
    grad[7, 0], y[7, 0] = float("nan"), -1.0        # this one is masked away
    grad[8, 9] = -0.0
    y[8, 9] = 1.0
    mask = DT.sign_mask_torch(y)
    out, bias = DT.bias_grad_torch(grad, mask)
    assert out.dtype == torch.float16 and bias.dtype == torch.float32
    want = torch.where(y > 0, grad.double(), torch.zeros((), dtype=torch.float64))
    assert torch.equal(out.double().nan_to_num(nan=-7.0), want.nan_to_num(nan=-7.0))
    # bits are moved: -0 stays -0 where the bit is set, a cleared element is +0
    assert out.view(torch.int16)[8, 9] == -32768 and out.view(torch.int16)[7, 0] == 0 and out.view(torch.int16)[3, 2] == 0
    assert torch.isnan(bias[3]) and torch.isinf(bias[6])
    clean = [c for c in range(C) if c not in (3, 6)]
    assert torch.isfinite(bias[clean]).all()
    # Half values are exact in fp32: only the n_pix - 1 fp32 additions round
    bound = n_pix * 2.0 ** -24 * want.abs().sum(0)[clean]
    assert ((bias[clean].double() - want.sum(0)[clean]).abs() <= bound).all()
    out3, bias3 = DT.bias_grad_torch(grad[:, :3])
    assert out3.data_ptr() == grad[:, :3].data_ptr() and bias3.dtype == torch.float32
    assert torch.equal(bias3[1:3].double(), grad[:, 1:3].float().sum(0).double())


def test_depth_with_eight_channels_per_lane():
    # csrc/dib_deblur_train.hip, "THE SUMMATION ORDER": QB = min(C / V, 256), R = 256 / QB, S = ceil(n_pix / (16 R)) <= 1024,
    # L = ceil(ceil(n_pix / S) / R); depth = L + ceil(log2 R) + S - 1
    assert DT.bias_grad_depth(5, 64, V=8) == 1 + 5 + 0                   # QB = 8, R = 32 rows, one slice of 5 pixels: L = 1
    assert DT.bias_grad_depth(4099, 64, V=8) == 15 + 5 + 8               # S = ceil(4099 / 512) = 9 slices of <= 456 pixels: L = ceil(456 / 32) = 15
    assert DT.bias_grad_depth(4099, 8, V=8) == 9 + 8 + 1                 # QB = 1, R = 256, S = ceil(4099 / 4096) = 2 slices of <= 2050: L = 9
    assert DT.bias_grad_depth(257, 3, V=1) == 4 + 7 + 0                  # 3 channels: one per lane, as the fp32 form
    assert DT.bias_grad_lanes(64, torch.float16) == 8 and DT.bias_grad_lanes(12, torch.float16) == 1 and DT.bias_grad_lanes(12, torch.float32) == 4
    # the default keeps today's values
    assert DT.bias_grad_depth(4099, 64) == DT.bias_grad_depth(4099, 64, V=4) == 16 + 4 + 16
    assert DT.bias_grad_depth(257, 3) == 4 + 7 + 0
    with pytest.raises(ValueError):
        DT.bias_grad_depth(5, 12, V=8)


def test_half_levels_and_the_autocast_forward():
    torch.manual_seed(0)
    model = deblur.MSResNet(n_scales=2, n_resblocks=2, n_feats=8, kernel_size=5)
    g = torch.Generator().manual_seed(3)
    patches = torch.rand(2, 3, 16, 16, generator=g)
    l32, l16 = DT.patch_levels(patches, 2), DT.patch_levels(patches, 2, torch.float16)
    assert [tuple(l.shape) for l in l16] == [(2, 6, 16, 16), (2, 3, 8, 8)] and all(l.dtype == torch.float16 for l in l16)
    assert all(l.is_contiguous(memory_format=torch.channels_last) for l in l16)
    for a, b in zip(l32, l16):
        assert torch.equal(a[:, :3].half(), b[:, :3])
    out = DT.msresnet_train_forward(model, l16)
    assert model.last_path == "torch-amp" and all(o.dtype == torch.float16 for o in out)
    DT.msresnet_train_forward(model, l32)
    assert model.last_path == "torch"                                          # fp32 levels: as before
    # the restatement of the HIP path's arithmetic runs anywhere, and differs from autocast by Half roundings only
    rest = DT.forward_amp_restated(model, l16)
    for o, r in zip(out, rest):
        assert r.dtype == torch.float16 and torch.allclose(o.float(), r.float(), rtol=0, atol=0.5)
    with pytest.raises(ValueError):
        DT.patch_levels(patches, 2, torch.bfloat16)


# ---- the driver -----------------------------------------------------------------------------------------------------------------

def _argv(out_dir, *extra):
    return ["--synthetic", "--synthetic_images", "4", "--synthetic_size", "40", "56", "--device", "cpu", "-j", "0", "-b", "2",
            "--patch_size", "16", "--print_freq", "1", "--output_dir", str(out_dir)] + TINY + list(extra)


def _run(out_dir, *extra):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        trainer = TD.main(_argv(out_dir, *extra))
    return buf.getvalue(), trainer


def _weights(path):
    return torch.load(path, map_location="cpu", weights_only=True)["G"]


def test_amp_driver_checkpoints_and_printed_lines(tmp_path):
    text, trainer = _run(tmp_path, "--epochs", "1", "--amp")
    lines = [l for l in text.splitlines() if "loss:" in l]
    assert len(lines) == 2 and all("path: torch-amp" in l and re.search(r"scale: [0-9.e+]+$", l) for l in lines), text[-1500:]
    assert "scale: 1024" in lines[0]
    assert trainer.optimizer._step_supports_amp_scaling and trainer.optimizer.defaults["fused"]
    ck = torch.load(tmp_path / "optim" / "optim-1.pt", map_location="cpu", weights_only=False)
    assert "scaler" in ck and ck["scaler"]["scale"] == 1024.0 and ck["args"]["amp"] is True
    state = torch.load(tmp_path / "models" / "model-1.pt", map_location="cpu", weights_only=True)
    assert set(state) == {"G"} and all(v.dtype == torch.float32 for v in state["G"].values())
    with contextlib.redirect_stdout(io.StringIO()):
        d = deblur.Deblurer(str(tmp_path))                                     # strict load
    out = d.deblur_(torch.rand(3, 20, 28))
    assert out.shape == (3, 20, 28) and torch.isfinite(out).all()
    # without --amp: no scale in the line, no scaler in the file, the optimizer as it was built before
    text, trainer = _run(tmp_path / "plain", "--epochs", "1")
    assert "scale:" not in text and "path: torch  " not in text and "path: torch\n" in text
    assert trainer.scaler is None and not trainer.optimizer.defaults["fused"]
    ck = torch.load(tmp_path / "plain" / "optim" / "optim-1.pt", map_location="cpu", weights_only=False)
    assert set(ck) == {"optimizer", "lr_scheduler", "epoch", "args"}


def test_amp_resume_gives_the_weights_of_the_uninterrupted_run(tmp_path):
    _run(tmp_path / "a", "--epochs", "2", "--save_every", "1", "--amp")
    _run(tmp_path / "b", "--epochs", "1", "--save_every", "1", "--amp")
    text, _ = _run(tmp_path / "b", "--epochs", "2", "--save_every", "1", "--amp", "--resume")
    assert "Resumed from" in text and "Epoch: [2]" in text and "Epoch: [1]" not in text
    a, b = _weights(tmp_path / "a" / "models" / "model-2.pt"), _weights(tmp_path / "b" / "models" / "model-2.pt")
    first = _weights(tmp_path / "a" / "models" / "model-1.pt")
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert any(not torch.equal(a[k], first[k]) for k in a)                     # the second epoch did train
    # the flag must be the one the file was written with, either way
    with pytest.raises(SystemExit, match="with --amp"):
        _run(tmp_path / "b", "--epochs", "3", "--resume")
    _run(tmp_path / "c", "--epochs", "1", "--save_every", "1")
    with pytest.raises(SystemExit, match="without --amp"):
        _run(tmp_path / "c", "--epochs", "2", "--amp", "--resume")


def test_init_scale_without_amp_is_refused():
    with pytest.raises(SystemExit, match="init_scale"):
        TD.main(["--synthetic", "--init_scale", "7"])
    with pytest.raises(SystemExit, match="init_scale"):
        TD.main(["--synthetic", "--amp", "--init_scale", "0"])
    args = TD.build_parser().parse_args(["--synthetic"])
    assert args.amp is False and args.init_scale == 1024.0


def test_every_step_is_skipped_at_a_scale_of_two_to_the_sixty(tmp_path):
    three = ("--synthetic_images", "6", "--epochs", "1", "--amp")              # 3 steps of 2 images
    text, trainer = _run(tmp_path / "big", *three, "--init_scale", "1152921504606846976")
    losses = [float(v) for v in re.findall(r"loss: ([0-9.einfa+-]+)", text)]
    assert len(losses) == 3 and all(torch.isfinite(torch.tensor(losses))), text[-1500:]     # the printed loss is the unscaled one
    assert trainer.scaler.get_scale() == 2.0 ** 57                             # halved after each of the three overflows
    args = TD.build_parser().parse_args(_argv(tmp_path / "big", *three, "--init_scale", "1152921504606846976"))
    TD.reject(args)
    args.distributed = False
    fresh = TD.Trainer(args, torch.device("cpu")).bare.state_dict()            # the same arguments, never stepped
    saved = _weights(tmp_path / "big" / "models" / "model-1.pt")
    assert set(saved) == set(fresh) and all(torch.equal(saved[k], fresh[k]) for k in fresh)
    # the same run at the default scale does train
    _, trainer = _run(tmp_path / "default", *three)
    moved = _weights(tmp_path / "default" / "models" / "model-1.pt")
    assert trainer.scaler.get_scale() == 1024.0 and any(not torch.equal(moved[k], fresh[k]) for k in fresh)
