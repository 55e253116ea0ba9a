"""`--deblur_first` on the host (reference engine.py:319-322, evaluate.py:240-243, models/deblur/): the network against the reference's
own MSResNet (a recorded fixture), the torch path's quantise / pad / pyramid against a float64 restatement on scipy, the stage composed
by hand, the checkpoint layout, the drivers and the engine's hand-over to the detector.

`python tests/test_deblur_first.py --write` rewrites tests/golden/deblur_pins.npz from the live reference's
models/deblur/MSResNet.py on CPU (DIB_REFERENCE_ROOT, default /root/reference): a seeded state dict (n_feats 8, n_resblocks 2, k 5,
n_scales 3), a seeded input pyramid at 24x32 / 12x16 / 6x8 and the three outputs.  Data only."""
import contextlib
import copy
import io
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "deblur_pins.npz")
TINY = dict(n_feats=8, n_resblocks=2, kernel_size=5, n_scales=3)
SIZES = [(5, 6), (37, 50), (64, 96)]        # 5x6 pads to 8x8, its coarsest level is 2x2: the 3-pixel halo is longer than the image


def write_fixture():
    import types
    sys.path.insert(0, os.environ.get("DIB_REFERENCE_ROOT", "/root/reference"))
    from models.deblur.MSResNet import MSResNet as Reference
    torch.manual_seed(20261019)
    net = Reference(types.SimpleNamespace(rgb_range=255, **TINY)).eval()
    with torch.no_grad():
        for p in net.parameters():                      # beyond the default init's range: biases and weights that move the output
            p.mul_(1.5)
    pyr = [torch.rand(1, 3, 24 >> s, 32 >> s) * 255 for s in range(3)]
    with torch.no_grad():
        out = net([p.clone() for p in pyr])
    data = {"sd/" + k: v.numpy() for k, v in net.state_dict().items()}
    data.update({"in%d" % s: pyr[s].numpy() for s in range(3)})
    data.update({"out%d" % s: out[s].numpy() for s in range(3)})
    np.savez_compressed(FIXTURE, **data)
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes,", len(data), "arrays")


@pytest.fixture(scope="module")
def pins():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def fixture_state(pins):
    return {k[3:]: torch.from_numpy(v.copy()) for k, v in pins.items() if k.startswith("sd/")}


@pytest.fixture(scope="module")
def tiny_dir(tmp_path_factory):
    from detectinblur_amd.models.deblur import write_random_checkpoint
    d = tmp_path_factory.mktemp("deblurrer")
    write_random_checkpoint(str(d), n_feats=8, n_resblocks=2, seed=3)
    return str(d)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


# ---- the float64 restatement of steps 1-3 (shared with the GPU tests) --------------------------------------------------------------

def pyramid_float64(q, n_scales=3):
    """q: integer-valued [3, H, W] array -> edge pad to a multiple of 2 ** (n_scales - 1), then per level
    scipy.ndimage.gaussian_filter(channel, 2 / 3, mode="reflect") and the mean of each 2 x 2 block, all in float64."""
    from scipy import ndimage
    d = 2 ** (n_scales - 1)
    q = np.asarray(q, dtype=np.float64)
    q = np.pad(q, ((0, 0), (0, -q.shape[1] % d), (0, -q.shape[2] % d)), mode="edge")
    levels = [q]
    for _ in range(1, n_scales):
        s = np.stack([ndimage.gaussian_filter(ch, 2 / 3, mode="reflect") for ch in levels[-1]])
        levels.append((s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2]) / 4)
    return levels


def every_half_in_unit_interval():
    """every Half value in [0, 1] (both zeros included), as a [3, 1, n] image"""
    bits = np.arange(0, 0x3C00 + 1, dtype=np.uint16)
    v = np.concatenate([bits.view(np.float16), np.array([-0.0], dtype=np.float16)])
    return torch.from_numpy(np.ascontiguousarray(np.broadcast_to(v, (3, 1, v.size))))


def make_image(h, w, dtype, seed=0):
    g = torch.Generator().manual_seed(1000 * h + w + seed)
    return torch.rand(3, h, w, generator=g).to(dtype)


# ---- the network -----------------------------------------------------------------------------------------------------------------------

def test_state_dict_is_the_references_and_loads_strictly(pins):
    from detectinblur_amd.models.deblur import MSResNet
    state = fixture_state(pins)
    assert len(state) == 40
    net = MSResNet(**TINY)
    own = net.state_dict()
    assert list(own) == list(state) and all(own[k].shape == state[k].shape for k in state)
    net.load_state_dict(state, strict=True)
    inferred = MSResNet.from_state_dict(state)
    assert (inferred.n_scales, inferred.n_resblocks, inferred.n_feats, inferred.kernel_size) == (3, 2, 8, 5)
    big = MSResNet()                                                      # the defaults are DeepDeblur's
    assert (big.n_scales, big.n_resblocks, big.n_feats, big.kernel_size) == (3, 19, 64, 5)
    assert big.state_dict()["body_models.2.body.0.weight"].shape == (64, 3, 5, 5) and big.state_dict()["body_models.0.body.0.weight"].shape == (64, 6, 5, 5)
    assert big.state_dict()["conv_end_models.1.uppath.0.weight"].shape == (12, 3, 5, 5) and "body_models.1.body.19.body.2.bias" in big.state_dict()


def test_network_outputs_equal_the_references(pins):
    from detectinblur_amd.models.deblur import MSResNet
    net = MSResNet.from_state_dict(fixture_state(pins)).eval()
    inputs = [torch.from_numpy(pins["in%d" % s].copy()) for s in range(3)]
    with torch.no_grad():
        out = net(inputs)
    for s in range(3):
        assert np.array_equal(inputs[s].numpy(), pins["in%d" % s])        # the inputs are left alone
        err = float(np.abs(out[s].numpy() - pins["out%d" % s]).max())
        print("level", s, "max abs error", err)
        assert out[s].shape == inputs[s].shape and err <= 1e-4
    assert float(np.abs(pins["out0"] - pins["in0"]).max()) > 1.0          # the network does something


# ---- steps 1-3 ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_torch_pyramid_equals_the_float64_restatement(size):
    """two 7-tap fp32 passes and a 4-term mean per level, two levels, values <= 255: errors of a few 1e-5; the bound is 1e-3"""
    from detectinblur_amd.models import deblur as D
    h, w = size
    x = make_image(h, w, torch.float32)
    q = D.quantise(x)
    assert np.array_equal(q.numpy(), np.trunc(x.numpy() * np.float32(255)))
    padded = D.pad_to_multiple(q, 4)
    want = pyramid_float64(q.numpy())
    assert tuple(padded.shape) == want[0].shape and padded.shape[1] % 4 == 0 and padded.shape[2] % 4 == 0
    assert np.array_equal(padded.numpy(), want[0])
    got = D.pyramid(padded, 3)
    assert [tuple(l.shape) for l in got] == [l.shape for l in want] and got[2].shape[1] == padded.shape[1] // 4
    for s in range(3):
        err = float(np.abs(got[s].numpy() - want[s]).max())
        print(size, "level", s, err)
        assert got[s].dtype == torch.float32 and err <= 1e-3
    assert float(np.abs(got[1].numpy() - want[0][:, 0::2, 0::2]).max()) > 1.0       # smoothing and averaging happened


def test_reflection_is_periodic():
    from detectinblur_amd.models.deblur import reflect_indices
    assert reflect_indices(2).tolist() == [1, 1, 0, 0, 1, 1, 0, 0]                  # d c b a | a b c d at n = 2, radius 3
    assert reflect_indices(5).tolist() == [2, 1, 0, 0, 1, 2, 3, 4, 4, 3, 2]


def test_quantisation_of_every_half_value():
    from detectinblur_amd.models.deblur import quantise
    x = every_half_in_unit_interval()
    got = quantise(x)
    want = np.trunc((x.numpy() * np.float16(255)).astype(np.float16).astype(np.float32))     # numpy rounds the Half product to Half
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    assert quantise(torch.tensor([[[0.50195312]]] * 3, dtype=torch.float16))[0, 0, 0] == 128
    assert quantise(torch.tensor([[[0.50195312]]] * 3, dtype=torch.float32))[0, 0, 0] == 127
    x32 = x.float()
    assert np.array_equal(quantise(x32).numpy(), np.trunc(x32.numpy() * np.float32(255)))
    assert (got != quantise(x32)).any()                                   # the Half rounding matters
    odd = torch.tensor([float("nan"), -0.5, 2.0, float("inf"), -float("inf")]).reshape(1, 1, -1).expand(3, 1, -1)
    assert quantise(odd)[0, 0].tolist() == [0, 0, 255, 255, 0]            # this library's choice outside [0, 1]


# ---- the stage -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_deblur_equals_the_steps_composed_by_hand(tiny_dir, dtype):
    from detectinblur_amd.models import deblur as D
    d = quiet(D.Deblurer, tiny_dir)
    assert not d.training and all(p.dtype == torch.float32 and not p.requires_grad for p in d.parameters())
    h, w = 37, 50
    x = make_image(h, w, dtype)
    got = d.deblur_(x)
    assert d.last_path == "torch" and got.dtype == torch.float32 and tuple(got.shape) == (3, h, w)
    levels = D.pyramid(D.pad_to_multiple(D.quantise(x), 4), 3)
    with torch.no_grad():
        out = d.model([l[None] for l in levels])[0]
    want = (out[0, :, :h, :w] + 0.5).clamp(0, 255) / 255
    assert torch.equal(got, want) and 0 <= float(got.min()) and float(got.max()) <= 1
    assert float((got - x.float()).abs().max()) > 0.01                    # a random network changes the image
    # the reference's method: the uint8 array in, the 0..255 tensor out, before the + 0.5
    arr = (x * 255).permute(1, 2, 0).to(torch.uint8).numpy()
    raw = d.deblurImage(arr)
    assert tuple(raw.shape) == (1, 3, h, w) and raw.dtype == torch.float32 and torch.equal(raw[0], out[0, :, :h, :w])
    assert torch.equal(raw.clone().add_(0.5).clamp_(0, 255) / 255, got[None])
    with pytest.raises(ValueError):
        d.deblur_(x[None])


def test_checkpoints_round_trip_and_the_epoch_choice_is_the_references(tmp_path):
    from detectinblur_amd.models import deblur as D
    a = D.write_random_checkpoint(str(tmp_path / "a"), n_feats=8, n_resblocks=1, n_scales=2, kernel_size=3, seed=1)
    assert a == str(tmp_path / "a" / "models" / "model-1.pt")
    saved = torch.load(a, weights_only=True)
    assert list(saved) == ["G"]
    for loc in (str(tmp_path / "a"), a):
        d = quiet(D.Deblurer, loc)
        assert (d.model.n_scales, d.model.n_resblocks, d.model.n_feats, d.model.kernel_size) == (2, 1, 8, 3) and d.checkpoint == a
        assert all(torch.equal(v, saved["G"][k]) for k, v in d.model.state_dict().items())
    again = D.write_random_checkpoint(str(tmp_path / "b"), n_feats=8, n_resblocks=1, n_scales=2, kernel_size=3, seed=1)
    other = D.write_random_checkpoint(str(tmp_path / "c"), n_feats=8, n_resblocks=1, n_scales=2, kernel_size=3, seed=2)
    first = "body_models.0.body.0.weight"
    assert torch.equal(torch.load(again, weights_only=True)["G"][first], saved["G"][first])
    assert not torch.equal(torch.load(other, weights_only=True)["G"][first], saved["G"][first])
    # models/model-9.pt and model-10.pt: the reference takes the LAST name of sorted(os.listdir(...)), a string sort
    D.write_random_checkpoint(str(tmp_path / "d"), n_feats=4, n_resblocks=1, n_scales=1, kernel_size=3, seed=9, epoch=9)
    D.write_random_checkpoint(str(tmp_path / "d"), n_feats=8, n_resblocks=1, n_scales=1, kernel_size=3, seed=10, epoch=10)
    names = sorted(os.listdir(tmp_path / "d" / "models"))
    assert names[-1] == "model-9.pt"
    d = quiet(D.Deblurer, str(tmp_path / "d"))
    assert d.checkpoint.endswith("model-9.pt") and d.model.n_feats == 4 and d.n_scales == 1
    with pytest.raises(FileNotFoundError):
        D.Deblurer(str(tmp_path / "nowhere"))


def test_write_random_command_line(tmp_path, monkeypatch, capsys):
    from detectinblur_amd.models import deblur as D
    monkeypatch.setattr(sys, "argv", ["deblur", "--write_random", str(tmp_path), "--n_feats", "4", "--n_resblocks", "1", "--seed", "5"])
    D._main()
    assert capsys.readouterr().out.strip() == str(tmp_path / "models" / "model-1.pt")
    assert quiet(D.Deblurer, str(tmp_path)).model.n_feats == 4


# ---- drivers ----------------------------------------------------------------------------------------------------------------------------

def test_both_parsers_accept_the_flags():
    from detectinblur_amd import evaluate as EV
    from detectinblur_amd import train as TR
    assert "deblur_first" not in TR._OUT_OF_SCOPE and "unfrozen_batch_norm" in TR._OUT_OF_SCOPE and "blurred_dataset" in TR._OUT_OF_SCOPE
    for parser in (TR.build_parser(), EV.build_parser()):
        a = parser.parse_args(["--synthetic", "--deblur_first", "--deblurer_model_location", "X"])
        assert a.deblur_first and a.deblurer_model_location == "X"
        TR.reject_out_of_scope(a)
        assert parser.parse_args([]).deblurer_model_location is None and not parser.parse_args([]).deblur_first
        for action in parser._actions:
            if action.dest in ("deblur_first", "deblurer_model_location"):
                assert "not built" not in action.help


def test_evaluate_main_without_a_location_names_both_flags():
    from detectinblur_amd import evaluate as EV
    args = EV.build_parser().parse_args(["--synthetic", "--device", "cpu", "--deblur_first"])
    with pytest.raises(SystemExit) as e, contextlib.redirect_stdout(io.StringIO()):
        EV.main(args)
    assert "--deblur_first" in str(e.value) and "--deblurer_model_location" in str(e.value)


def test_train_main_says_that_only_evaluate_reads_the_flag(monkeypatch, capsys):
    from detectinblur_amd import train as TR

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop()
    monkeypatch.setattr(TR.utils, "init_distributed_mode", stop)
    with pytest.raises(Stop):
        TR.main(TR.build_parser().parse_args(["--synthetic", "--device", "cpu", "--deblur_first", "--deblurer_model_location", "X"]))
    lines = [l for l in capsys.readouterr().out.splitlines() if "--deblur_first" in l]
    assert len(lines) == 1 and "evaluate.py" in lines[0]


def test_evaluate_main_runs_a_cell_on_the_host(tiny_dir, tmp_path, monkeypatch):
    from detectinblur_amd import evaluate as EV
    from detectinblur_amd.models import deblur as D
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(EV, "SWEEP_PARAMS", EV.SWEEP_PARAMS[:1])
    monkeypatch.setattr(EV, "SWEEP_FRACTIONS", EV.SWEEP_FRACTIONS[2:3])
    calls = []
    real = D.Deblurer.deblur_

    def counted(self, image):
        out = real(self, image)
        calls.append((tuple(image.shape), image.dtype, tuple(out.shape), out.dtype, self.last_path))
        return out
    monkeypatch.setattr(D.Deblurer, "deblur_", counted)
    args = EV.build_parser().parse_args(["--synthetic", "--synthetic_size", "128", "160", "--min_size", "128", "--max_size", "160", "--device", "cpu",
                                         "--blur_eval", "--cpu_blur", "--early_stop", "1", "--tensorboard_path", "", "--deblur_first",
                                         "--deblurer_model_location", tiny_dir])
    res = quiet(EV.main, args)
    assert len(res) == 1 and len(list(res.values())[0]["detections"]) == 2         # early_stop 1: images 0 and 1, as the reference counts
    assert calls == [((3, 128, 160), torch.float16, (3, 128, 160), torch.float32, "torch")] * 2


# ---- engine.evaluate ---------------------------------------------------------------------------------------------------------------------

class Recorder(object):
    """stands in for the Deblurer: records what the engine hands it and what it hands back"""

    def __init__(self, real):
        self.real, self.inputs, self.outputs = real, [], []

    def deblur_(self, image):
        self.inputs.append(image.clone())
        out = self.real.deblur_(image)
        self.outputs.append(out.clone())
        return out


def _loader(h, w, n, blur):
    from detectinblur_amd import utils
    from detectinblur_amd.coco_utils import SyntheticCocoDetection
    from detectinblur_amd.train import get_transform
    tf = get_transform(False, blur=True, blur_type=0.005, blur_ratio=1, blur_exposure=1 / 5, cpu_blur=True) if blur else get_transform(False)
    np.random.seed(11)
    ds = SyntheticCocoDetection(num_images=n, size=(h, w), boxes_per_image=2, transforms=tf, as_tensor=not blur)

    class L(list):
        dataset = ds
    return L(utils.collate_fn([ds[i]]) for i in range(n))


@pytest.mark.parametrize("mode", ["blurring_images", "vanilla_eval"])
def test_engine_hands_the_detector_the_deblurred_image(tiny_dir, mode):
    from detectinblur_amd import engine
    from detectinblur_amd.models.deblur import Deblurer
    from tests.test_overlay import FixedDetector, fixed_detections
    h, w, n = 70, 90, 2
    real = quiet(Deblurer, tiny_dir)
    loader = _loader(h, w, n, blur=mode == "blurring_images")
    kw = {mode: True}

    def run(**extra):
        model = FixedDetector(fixed_detections(h, w))
        batches = type(loader)(copy.deepcopy(list(loader)))
        quiet(engine.evaluate, model, batches, torch.device("cpu"), **kw, **extra)
        return model.seen
    plain = run()                                                         # deblur_first=False: the image as it was
    spy = Recorder(real)
    assert len(run(deblur_first=False, deblurer=spy)) == n and spy.inputs == []
    seen = run(deblur_first=True, deblurer=spy)
    assert len(seen) == n and len(spy.inputs) == n
    for i in range(n):
        assert spy.inputs[i].dtype == torch.float16 and torch.equal(spy.inputs[i].float(), plain[i])      # the (blurred) image, untouched
        assert seen[i].dtype == torch.float32 and tuple(seen[i].shape) == (3, h, w)
        assert torch.equal(seen[i], spy.outputs[i]) and torch.equal(seen[i], real.deblur_(spy.inputs[i]))
        assert not torch.equal(seen[i], plain[i])
    if mode == "blurring_images":                                         # the loader's blur did run: the input is not the sharp image
        sharp = _loader(h, w, n, blur=False)
        assert not torch.equal(plain[0], sharp[0][0][0].half().float())
    # a pass that neither blurs nor is the vanilla one never runs the stage (reference engine.py:319)
    neither = Recorder(real)
    model = FixedDetector(fixed_detections(h, w))
    quiet(engine.evaluate, model, type(loader)(copy.deepcopy(list(loader))), torch.device("cpu"), deblur_first=True, deblurer=neither)
    assert neither.inputs == [] and len(model.seen) == n
    with pytest.raises(ValueError, match="deblurer"):
        quiet(engine.evaluate, FixedDetector(fixed_detections(h, w)), loader, torch.device("cpu"), deblur_first=True, **kw)

# ---- the C entry points ----------------------------------------------------------------------------------------------------------------

def check_argument_errors():
    """null pointers, H or W < 1, n_scales outside 1..4, a padded size below the image: DIB_EINVAL with a message and no GPU call (the
    pointers below are never dereferenced: every call fails its checks first)"""
    from detectinblur_amd import _lib
    l = _lib.lib()
    fake, E = 4096, _lib.DIB_EINVAL
    lv = _lib.ptr_array([fake, fake, fake, fake])

    def pyr(in_dev=fake, dtype=_lib.DIB_F16, H=8, W=8, n=3, levels=lv):
        return l.dib_deblur_pyramid(in_dev, dtype, H, W, n, levels, None)
    for kw in (dict(in_dev=None), dict(levels=None), dict(levels=_lib.ptr_array([fake, None, fake]))):
        assert pyr(**kw) == E and b"null pointer" in l.dib_last_error(), kw
    for kw in (dict(H=0), dict(W=0), dict(H=-3)):
        assert pyr(**kw) == E and b"H, W >= 1" in l.dib_last_error(), kw
    for n in (0, 5, -1):
        assert pyr(n=n) == E and b"n_scales" in l.dib_last_error(), n
    assert pyr(dtype=7) == E and b"dtype" in l.dib_last_error()
    assert pyr(H=1 << 16, W=(1 << 14) + 1) == E and b"2^30" in l.dib_last_error()
    assert pyr(levels=_lib.ptr_array([fake + 4, fake, fake])) == E and b"aligned" in l.dib_last_error()

    def shuf(in_dev=fake, bias=fake, out=fake, h=2, w=2):
        return l.dib_deblur_shuffle_concat(in_dev, bias, out, h, w, None)
    for kw in (dict(in_dev=None), dict(bias=None), dict(out=None)):
        assert shuf(**kw) == E and b"null pointer" in l.dib_last_error(), kw
    assert shuf(h=0) == E and b"h, w >= 1" in l.dib_last_error() and shuf(w=-1) == E
    assert shuf(in_dev=fake + 4) == E and b"aligned" in l.dib_last_error()

    def fin(in_dev=fake, bias=fake, out=fake, H=5, W=6, Hp=8, Wp=8):
        return l.dib_deblur_finish(in_dev, bias, out, H, W, Hp, Wp, None)
    for kw in (dict(in_dev=None), dict(bias=None), dict(out=None)):
        assert fin(**kw) == E and b"null pointer" in l.dib_last_error(), kw
    assert fin(H=0) == E and b"H, W >= 1" in l.dib_last_error() and fin(W=0) == E
    assert fin(Hp=4) == E and b"smaller" in l.dib_last_error() and fin(Wp=5) == E
    assert l.dib_abi_version() == 7


def test_argument_errors_are_reported_without_a_gpu():
    check_argument_errors()


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        write_fixture()
    else:
        sys.exit("usage: python tests/test_deblur_first.py --write")
