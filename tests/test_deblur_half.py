"""`--deblur_first --deblur_precision half` on the host: DeepDeblur's `--precision half` (reference models/deblur/deblurInterface.py:37,40,
52-53: the module and its input pyramid are cast to Half, so every op runs and rounds in Half).  The drivers' flag, the default path bit
for bit, the torch Half path against an op-by-op restatement written out here, the checkpoint left alone, the Half path's error against
the float64 stage, and -- first -- that the data the GPU tests of the Half kernels use can tell one rounding from two.

"half(v)" below is rounding to nearest even; a Half op is its fp32 result rounded once (what ATen computes for Half tensors)."""
import contextlib
import hashlib
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_deblur_first import FIXTURE, fixture_state, make_image, quiet, tiny_dir  # noqa: F401  (tiny_dir: a fixture)

SHAPES = [(5, 6), (37, 50), (70, 101), (64, 96)]              # tests/test_deblur_first_gpu.py's
# C, h, w: 15 lane vectors (less than one block); 936 (3 full blocks + 168 lanes); the one-element-per-lane form at the 3 channels a
# coarser scale ends in (351 elements: a full block and a partial one)
EPILOGUE_SHAPES = [(8, 3, 5), (64, 9, 13), (3, 9, 13)]


def h2f(t):
    """round to Half and back"""
    return t.half().float()


# ---- the data of the kernels' GPU tests (tests/test_deblur_half_gpu.py imports these) ------------------------------------------------

def epilogue_data(C, h, w):
    """y (a convolution's Half output, channels-last), b (the Half bias as an fp32 vector), r (the Half residual).  The first pixel's
    channels hold the special values: NaN, +-inf, -0 + -0, Half denormals, sums beyond 65504 (with the bias; with the residual)."""
    g = torch.Generator().manual_seed(C * 10000 + h * 100 + w)
    y = (torch.randn(1, C, h, w, generator=g) * 40).half()
    r = (torch.randn(1, C, h, w, generator=g) * 40).half()
    b = h2f(torch.randn(C, generator=g))
    denormal = 2.0 ** -24                                                  # the smallest Half denormal
    k = min(C, 8)
    b[:k] = torch.tensor([-0.0, denormal, 40.0, 0.5, -1.0, 3 * denormal, 0.25, -40.0])[:k]
    y[0, :k, 0, 0] = torch.tensor([-0.0, 0.0, 65504.0, float("nan"), float("inf"), -denormal, 60000.0, -65504.0]).half()[:k]
    r[0, :k, 0, 0] = torch.tensor([-0.0, denormal, 1.0, 1.0, -float("inf"), -denormal, 60000.0, -1.0]).half()[:k]
    y[0, :k, 0, 1] = torch.tensor([0.0, -denormal, -float("inf"), 1.0, 1.0, 0.0, -60000.0, 40.0]).half()[:k]
    r[0, :k, 0, 1] = torch.tensor([0.0, 0.0, float("inf"), float("nan"), 1.0, -3 * denormal, -60000.0, 0.0]).half()[:k]
    if C < 8:                                                              # NaN, inf - inf and the residual's overflow: second row
        y[0, :3, 1, 0] = torch.tensor([float("nan"), float("inf"), 60000.0]).half()
        r[0, :3, 1, 0] = torch.tensor([1.0, -float("inf"), 60000.0]).half()
    cl = torch.channels_last
    return y.contiguous(memory_format=cl), b, r.contiguous(memory_format=cl)


def epilogue_want(y, b, r=None, relu=False):
    """torch's Half ops in the reference's order, on the tensors' device: conv output + bias (the bias add of a Half convolution), then
    ReLU, or ResBlock's `res += x`"""
    t = y + b.half().reshape(1, -1, 1, 1)
    if r is not None:
        t += r
    return torch.relu(t) if relu else t


def finish_data(h, w):
    """the existing finish test's data as Half: raw [1, 3, Hp, Wp] in +-300 (v + 127.5 straddles 0 and 255) with its special values, and
    the bias as an fp32 vector of Half values"""
    hp, wp = -(-h // 4) * 4, -(-w // 4) * 4
    g = torch.Generator().manual_seed(h * 1000 + w)
    raw = torch.rand(1, 3, hp, wp, generator=g) * 600 - 300
    raw[0, 1, 0, 0], raw[0, 2, h - 1, w - 1], raw[0, 0, h // 2, w // 2] = float("nan"), float("inf"), -float("inf")
    raw[0, 0, 0, 1], raw[0, 1, 0, 1] = -128.0, 127.0                        # lands on the clamp's ends exactly (bias 0)
    bias = h2f(torch.tensor([0.0, 0.3, -7.25]))
    return raw.half().contiguous(memory_format=torch.channels_last), bias


def finish_want(raw, bias, h, w):
    """torch's Half ops: the last convolution's bias, MSResNet's + 127.5, the crop, `.add_(0.5).clamp_(0, 255) / 255`"""
    return ((raw + bias.half().reshape(1, -1, 1, 1)) + 127.5)[0, :, :h, :w].clone().add_(0.5).clamp_(0, 255) / 255


def differing_share(a, b):
    """share of elements whose Half bits differ (NaN positions left out)"""
    ok = ~(torch.isnan(a) | torch.isnan(b))
    return float((a.view(torch.int16) != b.view(torch.int16))[ok].float().mean())


# ---- the test inputs discriminate: first ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chw", EPILOGUE_SHAPES, ids=lambda s: "C%d_%dx%d" % s)
def test_epilogue_data_tells_two_roundings_from_one(chw):
    """half(half(y + b) + r) against half((y + b) + r) evaluated in fp32: on random data 28 % of the elements differ; the test data must
    show at least 5 %, or a kernel without the intermediate rounding would pass the bit-for-bit test"""
    y, b, r = epilogue_data(*chw)
    double = epilogue_want(y, b, r)
    single = ((y.float() + b.reshape(1, -1, 1, 1)) + r.float()).half()
    share = differing_share(double, single)
    print(chw, "share of elements where two roundings differ from one:", share)
    assert share >= 0.05


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_finish_data_tells_four_roundings_from_one(shape):
    """every op rounded to Half against the fp32 expression rounded once: 10 % of the elements differ on data straddling the clamp; at
    least 2 % must"""
    h, w = shape
    raw, bias = finish_data(h, w)
    double = finish_want(raw, bias, h, w)
    x = raw.float()[0, :, :h, :w] + bias.reshape(-1, 1, 1)
    single = (((x + 127.5) + 0.5).clamp(0, 255) * np.float32(1.0 / 255.0)).half()
    share = differing_share(double, single)
    print(shape, "share of elements where the Half ops differ from one rounding:", share)
    assert share >= 0.02


# ---- parsers and drivers -----------------------------------------------------------------------------------------------------------

def test_both_parsers_accept_the_flag_and_default_to_single():
    from detectinblur_amd import evaluate as EV
    from detectinblur_amd import train as TR
    for parser in (TR.build_parser(), EV.build_parser()):
        assert parser.parse_args([]).deblur_precision == "single"
        a = parser.parse_args(["--synthetic", "--deblur_first", "--deblurer_model_location", "X", "--deblur_precision", "half"])
        assert a.deblur_precision == "half" and a.deblur_first
        TR.reject_out_of_scope(a)
        TR.reject_out_of_scope(parser.parse_args(["--synthetic", "--deblur_precision", "single"]))      # the default does nothing: accepted
        with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
            parser.parse_args(["--deblur_precision", "bf16"])
        # the flag is independent of --amp: every combination parses and passes the checks
        b = parser.parse_args(["--synthetic", "--amp", "--deblur_first", "--deblurer_model_location", "X", "--deblur_precision", "half"])
        TR.reject_out_of_scope(b)
        assert b.amp and b.deblur_precision == "half"


@pytest.mark.parametrize("extra", [[], ["--amp"]], ids=["plain", "amp"])
def test_half_without_deblur_first_exits_naming_both_flags(extra):
    from detectinblur_amd import evaluate as EV
    from detectinblur_amd import train as TR
    args = EV.build_parser().parse_args(["--synthetic", "--device", "cpu", "--deblur_precision", "half"] + extra)
    with pytest.raises(SystemExit) as e, contextlib.redirect_stdout(io.StringIO()):
        EV.main(args)
    assert "--deblur_precision" in str(e.value) and "--deblur_first" in str(e.value) and "half" in str(e.value)
    with pytest.raises(SystemExit) as e:
        TR.reject_out_of_scope(TR.build_parser().parse_args(["--synthetic", "--deblur_precision", "half"]))
    assert "--deblur_precision" in str(e.value) and "--deblur_first" in str(e.value)


def test_train_main_says_that_only_evaluate_reads_the_flag(monkeypatch, capsys):
    from detectinblur_amd import train as TR

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop()
    monkeypatch.setattr(TR.utils, "init_distributed_mode", stop)
    with pytest.raises(Stop):
        TR.main(TR.build_parser().parse_args(["--synthetic", "--device", "cpu", "--deblur_first", "--deblurer_model_location", "X",
                                              "--deblur_precision", "half"]))
    lines = [l for l in capsys.readouterr().out.splitlines() if "--deblur_precision" in l]
    assert len(lines) == 1 and "evaluate.py" in lines[0]


def test_evaluate_passes_the_flag_through_and_amp_leaves_the_deblurrer_fp32(tiny_dir):
    from detectinblur_amd import evaluate as EV
    base = ["--synthetic", "--device", "cpu", "--deblur_first", "--deblurer_model_location", tiny_dir]
    parse = EV.build_parser().parse_args
    assert EV.build_deblurer(parse(["--synthetic", "--device", "cpu"]), torch.device("cpu")) is None
    for extra, precision, dtype in (([], "single", torch.float32), (["--amp"], "single", torch.float32),
                                    (["--deblur_precision", "half"], "half", torch.float16),
                                    (["--amp", "--deblur_precision", "half"], "half", torch.float16)):
        d = quiet(EV.build_deblurer, parse(base + extra), torch.device("cpu"))
        assert d.precision == precision and all(p.dtype == dtype for p in d.parameters()), extra
        assert d.deblur_(make_image(8, 8, torch.float16)).dtype == dtype


def test_evaluate_main_runs_a_cell_on_the_host_in_half(tiny_dir, tmp_path, monkeypatch):
    from detectinblur_amd import evaluate as EV
    from detectinblur_amd.models import deblur as D
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(EV, "SWEEP_PARAMS", EV.SWEEP_PARAMS[:1])
    monkeypatch.setattr(EV, "SWEEP_FRACTIONS", EV.SWEEP_FRACTIONS[2:3])
    calls = []
    real = D.Deblurer.deblur_

    def counted(self, image):
        out = real(self, image)
        calls.append((self.precision, image.dtype, tuple(out.shape), out.dtype, self.last_path))
        return out
    monkeypatch.setattr(D.Deblurer, "deblur_", counted)
    args = EV.build_parser().parse_args(["--synthetic", "--synthetic_size", "128", "160", "--min_size", "128", "--max_size", "160", "--device", "cpu",
                                         "--blur_eval", "--cpu_blur", "--early_stop", "1", "--tensorboard_path", "", "--deblur_first",
                                         "--deblurer_model_location", tiny_dir, "--deblur_precision", "half"])
    res = quiet(EV.main, args)
    assert len(res) == 1 and len(list(res.values())[0]["detections"]) == 2
    assert calls == [("half", torch.float16, (3, 128, 160), torch.float16, "torch")] * 2


# ---- the class -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixture_checkpoint(tmp_path_factory):
    """the network of tests/golden/deblur_pins.npz (n_feats 8, 2 blocks, k 5, 3 scales) as a checkpoint file"""
    with np.load(FIXTURE) as f:
        state = fixture_state({k: f[k] for k in f.files})
    path = str(tmp_path_factory.mktemp("fixture_net") / "fixture.pt")
    torch.save({"G": state}, path)
    return path


def test_precision_is_checked():
    from detectinblur_amd.models import deblur as D
    assert D.PRECISIONS == ("single", "half")
    for bad in ("bf16", "double", None, "Half", 16):
        with pytest.raises(ValueError, match="precision"):
            D.Deblurer("nowhere", precision=bad)                          # refused before the checkpoint is looked for


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_single_is_the_default_and_unchanged(fixture_checkpoint, dtype):
    """precision="single" against the steps composed from the module's own functions around a network built straight from the state dict,
    as tests/test_deblur_first.py composes them: bit for bit, fp32 parameters, fp32 out"""
    from detectinblur_amd.models import deblur as D
    h, w = 37, 50
    x = make_image(h, w, dtype)
    default, single = quiet(D.Deblurer, fixture_checkpoint), quiet(D.Deblurer, fixture_checkpoint, precision="single")
    assert default.precision == single.precision == "single"
    net = D.MSResNet.from_state_dict(torch.load(fixture_checkpoint, weights_only=True)["G"]).eval()
    with torch.no_grad():
        out = net([l[None] for l in D.pyramid(D.pad_to_multiple(D.quantise(x), 4), 3)])[0]
    want = (out[0, :, :h, :w] + 0.5).clamp(0, 255) / 255
    for d in (default, single):
        got = d.deblur_(x)
        assert got.dtype == torch.float32 and torch.equal(got, want) and d.last_path == "torch"
        assert all(p.dtype == torch.float32 for p in d.parameters())
        assert all(torch.equal(v, net.state_dict()[k]) for k, v in d.model.state_dict().items())


def half_stage_by_hand(state, x, n_scales=3, n_resblocks=2):
    """steps 1-5 under precision half, written out: the fp32 pyramid, then Half tensors and one torch op per op of the reference's graph.
    `state`: the fp32 state dict (cast here, as the reference casts the loaded module).  No call into MSResNet or Deblurer."""
    from detectinblur_amd.models import deblur as D
    h, w = x.shape[1:]
    W = {k: v.half() for k, v in state.items()}

    def conv(t, key):
        return F.conv2d(t, W[key + ".weight"], W[key + ".bias"], 1, W[key + ".weight"].shape[-1] // 2)
    levels = D.pyramid(D.pad_to_multiple(D.quantise(x), 2 ** (n_scales - 1)), n_scales)          # fp32, as the reference's host pyramid
    levels = [l[None].half() - 127.5 for l in levels]                                               # the upload's cast, then the Half mean shift
    t = levels[-1]
    for s in range(n_scales - 1, -1, -1):
        body = "body_models.%d.body." % s
        t = conv(t, body + "0")
        for i in range(1, n_resblocks + 1):
            res = conv(torch.relu(conv(t, body + "%d.body.0" % i)), body + "%d.body.2" % i)
            res += t
            t = res
        out = conv(t, body + "%d" % (n_resblocks + 1))
        if s > 0:
            up = F.pixel_shuffle(conv(out, "conv_end_models.%d.uppath.0" % s), 2)
            t = torch.cat((levels[s - 1], up), 1)
    net_out = out + 127.5
    assert net_out.dtype == torch.float16
    return net_out[:, :, :h, :w], (net_out[0, :, :h, :w].clone().add_(0.5).clamp_(0, 255) / 255)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_torch_half_path_equals_the_ops_written_out(fixture_checkpoint, dtype):
    from detectinblur_amd.models import deblur as D
    h, w = 37, 50
    x = make_image(h, w, dtype)
    digest = hashlib.sha256(open(fixture_checkpoint, "rb").read()).hexdigest()
    d = quiet(D.Deblurer, fixture_checkpoint, precision="half")
    assert not d.training and all(p.dtype == torch.float16 and not p.requires_grad for p in d.parameters())
    got = d.deblur_(x)
    assert d.last_path == "torch" and got.dtype == torch.float16 and tuple(got.shape) == (3, h, w)
    state = torch.load(fixture_checkpoint, weights_only=True)["G"]
    raw_want, want = half_stage_by_hand(state, x)
    assert torch.equal(got, want) and 0 <= float(got.min()) and float(got.max()) <= 1
    # it is a Half computation, not the fp32 one cast at the end
    single = quiet(D.Deblurer, fixture_checkpoint).deblur_(x)
    assert not torch.equal(got, single.half()) and float((got.float() - single).abs().max()) < 0.01
    # the reference's method: the uint8 array in, the Half 0..255 tensor out, before the + 0.5
    arr = (x * 255).permute(1, 2, 0).to(torch.uint8).numpy()
    raw = d.deblurImage(arr)
    assert tuple(raw.shape) == (1, 3, h, w) and raw.dtype == torch.float16 and torch.equal(raw, raw_want)
    assert torch.equal(raw.clone().add_(0.5).clamp_(0, 255) / 255, got[None])
    # the file is left alone: fp32, the reference's keys, loads strictly into a fresh fp32 module
    assert hashlib.sha256(open(fixture_checkpoint, "rb").read()).hexdigest() == digest
    again = torch.load(fixture_checkpoint, weights_only=True)["G"]
    assert all(v.dtype == torch.float32 for v in again.values()) and list(again) == list(d.model.state_dict())
    D.MSResNet(n_scales=3, n_resblocks=2, n_feats=8, kernel_size=5).load_state_dict(again, strict=True)
    assert all(torch.equal(v, again[k].half()) for k, v in d.model.state_dict().items())           # cast after loading, nothing else


def test_half_path_is_refused_by_the_hip_gate_on_the_host_and_for_widths_off_eight(tmp_path):
    from detectinblur_amd.models import deblur as D
    D.write_random_checkpoint(str(tmp_path), n_feats=12, n_resblocks=1, n_scales=2, kernel_size=3, seed=1)
    x = make_image(9, 10, torch.float16)
    half, single = quiet(D.Deblurer, str(tmp_path), precision="half"), quiet(D.Deblurer, str(tmp_path))
    assert not half._hip_ok(x) and half.deblur_(x).dtype == torch.float16 and half.last_path == "torch"

    class OnDevice(object):                                                # what _hip_ok asks of an image, with a CUDA one's answers
        is_cuda, dtype, shape, device = True, torch.float16, (3, 9, 10), next(half.model.parameters()).device

        def dim(self):
            return 3

        def numel(self):
            return 270
    assert single._hip_ok(OnDevice()) and not half._hip_ok(OnDevice())      # n_feats 12: % 4 == 0 but not % 8


# ---- accuracy ------------------------------------------------------------------------------------------------------------------------

def half_error(location, x):
    from detectinblur_amd.models import deblur as D
    from tests.test_deblur_first_gpu import float64_stage
    want = float64_stage(quiet(D.Deblurer, location), x)
    got = quiet(D.Deblurer, location, precision="half").deblur_(x)
    inside = float(((want > 0.02) & (want < 0.98)).mean())
    return float(np.abs(got.float().numpy() - want).max()), inside


def test_half_path_against_the_float64_stage(fixture_checkpoint, tmp_path):
    """Scale 0..1.  Measured on the CPU: the fixture's net at 37x50 7.8e-4, the real widths (64 features, 19 blocks, seed 0) at 36x52
    7.7e-4 (fp32: 3.6e-7 and 2.7e-7).  Bound: twice the larger, 1.6e-3 -- the factor covers another BLAS order of the convolution sums."""
    from detectinblur_amd.models.deblur import write_random_checkpoint
    write_random_checkpoint(str(tmp_path), seed=0)
    for name, location, x in (("fixture net 37x50", fixture_checkpoint, make_image(37, 50, torch.float16)),
                              ("real widths 36x52", str(tmp_path), make_image(36, 52, torch.float16))):
        err, inside = half_error(location, x)
        print(name, "Half torch path vs float64 stage:", err, "unsaturated share", inside)
        assert inside > 0.5 and 0 < err <= 1.6e-3


# ---- the C entry points --------------------------------------------------------------------------------------------------------------

def check_argument_errors_f16():
    """the Half forms refuse what the fp32 forms refuse, DIB_EINVAL with a message and no GPU call (the pointers are never dereferenced)"""
    from detectinblur_amd import _lib
    l = _lib.lib()
    fake, E = 4096, _lib.DIB_EINVAL
    lv = _lib.ptr_array([fake, fake, fake, fake])

    def pyr(in_dev=fake, dtype=_lib.DIB_F16, H=8, W=8, n=3, levels=lv, work=fake):
        return l.dib_deblur_pyramid_f16(in_dev, dtype, H, W, n, levels, work, None)
    for kw in (dict(in_dev=None), dict(levels=None), dict(levels=_lib.ptr_array([fake, None, fake])), dict(work=None), dict(work=None, n=4)):
        assert pyr(**kw) == E and b"null pointer" in l.dib_last_error(), kw
    for kw in (dict(H=0), dict(W=0), dict(H=-3)):
        assert pyr(**kw) == E and b"H, W >= 1" in l.dib_last_error(), kw
    for n in (0, 5, -1):
        assert pyr(n=n) == E and b"n_scales" in l.dib_last_error(), n
    assert pyr(dtype=7) == E and b"dtype" in l.dib_last_error()
    assert pyr(H=1 << 16, W=(1 << 14) + 1) == E and b"2^30" in l.dib_last_error()
    assert pyr(levels=_lib.ptr_array([fake + 8, fake, fake])) == E and b"aligned" in l.dib_last_error()
    assert pyr(work=fake + 4) == E and b"aligned" in l.dib_last_error()
    assert pyr(in_dev=fake + 1) == E and b"aligned" in l.dib_last_error()

    def shuf(in_dev=fake, bias=fake, out=fake, h=2, w=2):
        return l.dib_deblur_shuffle_concat_f16(in_dev, bias, out, h, w, None)
    for kw in (dict(in_dev=None), dict(bias=None), dict(out=None)):
        assert shuf(**kw) == E and b"null pointer" in l.dib_last_error(), kw
    assert shuf(h=0) == E and b"h, w >= 1" in l.dib_last_error() and shuf(w=-1) == E
    for kw in (dict(in_dev=fake + 8), dict(out=fake + 8), dict(bias=fake + 2)):
        assert shuf(**kw) == E and b"aligned" in l.dib_last_error(), kw

    def fin(in_dev=fake, bias=fake, out=fake, H=5, W=6, Hp=8, Wp=8):
        return l.dib_deblur_finish_f16(in_dev, bias, out, H, W, Hp, Wp, None)
    for kw in (dict(in_dev=None), dict(bias=None), dict(out=None)):
        assert fin(**kw) == E and b"null pointer" in l.dib_last_error(), kw
    assert fin(H=0) == E and b"H, W >= 1" in l.dib_last_error() and fin(W=0) == E
    assert fin(Hp=4) == E and b"smaller" in l.dib_last_error() and fin(Wp=5) == E
    for kw in (dict(in_dev=fake + 1), dict(out=fake + 1), dict(bias=fake + 2)):
        assert fin(**kw) == E and b"aligned" in l.dib_last_error(), kw

    def act(x=fake, bias=fake, res=None, n=64, C=8):
        return l.dib_bias_act_f16_nhwc(x, bias, res, n, C, 0, None)
    for kw in (dict(C=0), dict(n=-8), dict(n=20), dict(C=3, n=64)):
        assert act(**kw) == E and b"multiple of C" in l.dib_last_error(), kw
    for kw in (dict(x=None), dict(bias=None)):
        assert act(**kw) == E and b"null pointer" in l.dib_last_error(), kw
    for kw in (dict(x=fake + 1), dict(bias=fake + 2), dict(res=fake + 1)):
        assert act(**kw) == E and b"aligned" in l.dib_last_error(), kw
    assert act(n=0, x=None) == 0                                            # empty: nothing to do, as in the family
    assert l.dib_abi_version() == 7


def test_argument_errors_are_reported_without_a_gpu():
    check_argument_errors_f16()
