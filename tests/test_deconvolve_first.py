"""`--deconvolve_first` on the host: the Richardson-Lucy iteration of models/deconvolve.py (the torch restatement the drivers run under
`--device cpu`) against a float64 numpy statement of the definition written here, its behaviour, the C entry point's argument checks,
and the driver.  tests/test_deconvolve_first_gpu.py holds the HIP kernels to the same float64 reference, with the same tolerance rule.

The definition (include/dib.h, dib_rl_deconvolve).  Taps {(r_t, c_t, w_t)}: the PSF divided by its sum in its own dtype, non-zero entries
in row-major order; K the canvas, o = K / 2 - 1, pa = K / 2, pb = K / 2 - 1.
    (A  x)[i, j] = sum_t w_t x[m (i - (r_t - o)), m (j - (c_t - o))]    m: s == -pa -> n + pb first (the wrap), then the padding rule
    (A* u)[i, j] = sum_t w_t u[m'(i + (r_t - o)), m'(j + (c_t - o))]    m': the padding rule alone
    x_0 = y;  q = y / max(A x_k, eps);  x_{k+1} = clamp(x_k * A* q, 0, 1)
padding rule: K = 256 replicate; K = 128 zero when H < 64 or W < 64, else reflect (no edge repeat).

Tolerance of every comparison against float64: max(8 d, N 2^-20).  d = the largest deviation from float64 of a float32 numpy
restatement of the same case (computed here, at run time, from the reference alone); 2^-20 = 16 ulp of a value near 1 per iteration, the
worst-case order of a 40-tap fp32 sum of values <= 1; the factor 8 covers another tap order and fused multiply-adds, which move the
rounding by the same order as the restatement's own."""
import contextlib
import functools
import io
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

EPS = 1e-6
ITERATIONS = (1, 2, 5)


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


# ---- the float64 statement -----------------------------------------------------------------------------------------------------------

def ref_mode(K, H, W):
    if K > 129:
        return "replicate"
    return "zero" if (H < 64 or W < 64) else "reflect"


def ref_map(s, n, K, mode, wrap):
    """(source index, reads-zero) of the virtual coordinates s"""
    s = np.asarray(s, dtype=np.int64).copy()
    if wrap:
        s[s == -(K // 2)] = n + K // 2 - 1
    zero = np.zeros(s.shape, dtype=bool)
    if mode == "reflect":
        s = np.where(s < 0, -s, s)
        s = np.where(s > n - 1, 2 * (n - 1) - s, s)
    elif mode == "zero":
        zero = (s < 0) | (s > n - 1)
    return np.clip(s, 0, n - 1), zero


def ref_sweep(x, taps, K, adjoint, dtype=np.float64):
    rows, cols, weights = taps
    C, H, W = x.shape
    o, mode = K // 2 - 1, ref_mode(K, H, W)
    acc = np.zeros((C, H, W), dtype=dtype)
    i, j = np.arange(H), np.arange(W)
    for r, c, w in zip(rows, cols, weights):
        si, zi = ref_map(i + (r - o) if adjoint else i - (r - o), H, K, mode, not adjoint)
        sj, zj = ref_map(j + (c - o) if adjoint else j - (c - o), W, K, mode, not adjoint)
        g = x[:, si][:, :, sj]
        if mode == "zero":
            g = g * (~zi[None, :, None] & ~zj[None, None, :]).astype(dtype)
        acc = acc + dtype(w) * g
    return acc


def ref_rl(y, taps, K, iterations, eps=EPS, dtype=np.float64):
    y = np.asarray(y).astype(dtype)
    x = y
    for _ in range(iterations):
        q = y / np.maximum(ref_sweep(x, taps, K, False, dtype), dtype(eps))
        x = np.clip(x * ref_sweep(q, taps, K, True, dtype), dtype(0), dtype(1))
    return x


# ---- the cases -----------------------------------------------------------------------------------------------------------------------

def trace_psf(K, wrap_taps=True, length=40, swing=9):
    """a curved trace of `length` (40) taps around the canvas centre, plus (wrap_taps) one tap in the last row and one in the last column: the two
    that read the wrap row / column of the blur.  Values are small multiples of 2^-10: their sum is exact in fp16 and fp32 in any order,
    so every way of normalising gives the same weights."""
    psf = np.zeros((K, K), dtype=np.float64)
    c0 = K // 2 - 1
    for t in range(length):
        r = c0 + int(round(swing * np.sin(t / 9.0))) + t // 8
        psf[r, c0 - length // 2 + t] += (1 + (t * 5) % 7) / 1024.0
    if wrap_taps:
        psf[K - 1, c0 + 3] = 3 / 1024.0
        psf[c0 - 2, K - 1] = 2 / 1024.0
    return psf


def dense_psf(K=128):
    """the trace through a Gaussian of sigma 2 (a --dilate_psf-like PSF): more than 1,000 taps, many segments"""
    from scipy.ndimage import gaussian_filter
    psf = gaussian_filter(trace_psf(K, wrap_taps=False, length=64, swing=16), 2.0)
    psf[psf < 3e-7] = 0              # (what is left survives the rounding to Half: the smallest subnormal is 6e-8)
    return psf


def smooth_truth(C, H, W):
    i, j = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    return np.stack([0.525 + 0.475 * np.sin(0.23 * i + 0.7 * c) * np.cos(0.17 * j - 0.4 * c) for c in range(C)])


# name -> (C, H, W, K, PSF builder)
CASES = {
    "reflect": (3, 70, 90, 128, trace_psf),
    "reflect65": (3, 65, 65, 128, trace_psf),
    "zero": (3, 40, 50, 128, trace_psf),
    "replicate": (3, 70, 90, 256, trace_psf),
    "oneplane": (1, 67, 131, 128, trace_psf),
    "dense": (3, 70, 90, 128, dense_psf),
}
HOST_CASES = ("reflect", "zero", "replicate")


@functools.lru_cache(maxsize=None)
def case(name, psf_dtype="float16"):
    """dict: psf (K x K, psf_dtype, un-normalised), taps (rows, cols, float64 weights: the normalised PSF's, as the compaction writes
    them), truth (float64), y16 (the float64 blur of the truth rounded to Half, as the blur hands it on), K"""
    import dib_oracle as O
    C, H, W, K, build = CASES[name]
    psf = build(K)
    psf = O.to_half_like_torch(psf) if psf_dtype == "float16" else psf.astype(np.float32)
    norm = O.normalize_psf(psf)
    rows, cols, wts = O.taps_of(norm)
    taps = (rows, cols, wts.astype(np.float64))
    truth = smooth_truth(C, H, W)
    y16 = ref_sweep(truth, taps, K, False).astype(np.float16)
    return dict(psf=psf, taps=taps, truth=truth, y16=y16, K=K, shape=(C, H, W))


@functools.lru_cache(maxsize=None)
def reference(name, iterations, y_dtype="float16", psf_dtype="float16"):
    """(x_N in float64, tolerance) of a case: y is the Half image, or (y_dtype float32) its fp32 blur"""
    cs = case(name, psf_dtype)
    y = cs["y16"] if y_dtype == "float16" else ref_sweep(cs["truth"], cs["taps"], cs["K"], False).astype(np.float32)
    return reference_of(y, cs["taps"], cs["K"], iterations)


def reference_of(y, taps, K, iterations, eps=EPS):
    """(x_N in float64, tolerance, d) of one image and tap list: the tolerance rule of this module's docstring, stated once (the
    geometry cases of tests/test_deconvolve_geometry.py take it from here)"""
    want = ref_rl(y, taps, K, iterations, eps)
    d = float(np.abs(ref_rl(y, taps, K, iterations, eps, dtype=np.float32).astype(np.float64) - want).max())
    return want, max(8 * d, iterations * 2.0 ** -20), d


def torch_psf(cs):
    return torch.from_numpy(cs["psf"].copy())


# ---- 1, 2: the definition --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("iterations", ITERATIONS)
@pytest.mark.parametrize("name", HOST_CASES)
def test_torch_path_against_the_float64_definition(name, iterations):
    from detectinblur_amd.models import deconvolve as DC
    cs = case(name)
    want, tol, d = reference(name, iterations)
    got = DC.richardson_lucy(torch.from_numpy(cs["y16"].copy()), torch_psf(cs), iterations=iterations, eps=EPS)
    assert got.dtype == torch.float32 and tuple(got.shape) == cs["shape"] and not got.is_cuda
    err = float(np.abs(got.numpy().astype(np.float64) - want).max())
    print("%s N=%d: torch vs float64 %.3g, float32 restatement %.3g, tolerance %.3g" % (name, iterations, err, d, tol))
    assert err <= tol, (err, tol)


def test_taps_are_the_compactions():
    """the torch path's taps of a PSF = the oracle's normalised row-major list (what dib_psf_compact writes), wrap taps included"""
    from detectinblur_amd.models import deconvolve as DC
    cs = case("reflect")
    taps = DC.taps_of_psf(torch_psf(cs))
    rows, cols, wts = cs["taps"]
    assert len(taps) == 42 and taps.K == 128
    assert np.array_equal(taps.rows.numpy(), rows) and np.array_equal(taps.cols.numpy(), cols)
    assert np.array_equal(taps.weights.numpy().astype(np.float64), wts)
    assert 127 in rows and 127 in cols


# ---- 3: behaviour ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["reflect", "zero", "replicate"])
def test_forward_operator_is_the_blur(name):
    """A of this module = manual_blur: against the oracle's statement (padded image, rolls: another formulation, the wrap comes from
    the roll) in fp32 accumulation -- only rounding apart: T taps, each product and each sum rounded once in fp32 on values <= 1:
    at most 2 T 2^-24 -- and against the oracle's Half arithmetic, the blur the detector's image went through: the Half input
    (2^-12), T products of values <= 1 whose roundings add up to at most 2^-12 (the weights sum to 1), T sums rounded to Half
    (2^-12 each): (T + 2) 2^-12."""
    import dib_oracle as O
    from detectinblur_amd.models import deconvolve as DC
    cs = case(name)
    T = len(cs["taps"][0])
    x16 = cs["truth"].astype(np.float16)
    norm = O.normalize_psf(cs["psf"])
    a64 = ref_sweep(x16.astype(np.float64), cs["taps"], cs["K"], False)
    got = DC.forward_blur(torch.from_numpy(x16.copy()), torch_psf(cs)).numpy().astype(np.float64)
    assert np.abs(got - a64).max() <= 2 * T * 2.0 ** -24
    o32 = O.manual_blur(x16.astype(np.float32), norm.astype(np.float32), fp32_accumulate=True).astype(np.float64)
    assert np.abs(o32 - a64).max() <= 2 * T * 2.0 ** -24
    o16 = O.manual_blur(x16, norm).astype(np.float64)
    assert np.abs(o16 - a64).max() <= (T + 2) * 2.0 ** -12


def test_a_constant_image_stays_constant_in_the_interior():
    """the weights sum to 1 within Half rounding of the normalisation (s): A c = s c, q = 1 / s, A* q = 1 wherever no boundary rule
    is involved, so one iteration gives c s / s: c within a few fp32 ulp (the wrap taps only reach rows and columns 0)"""
    from detectinblur_amd.models import deconvolve as DC
    cs = case("reflect")
    C, H, W = cs["shape"]
    y = torch.full((C, H, W), 0.375, dtype=torch.float16)
    x = DC.richardson_lucy(y, torch_psf(cs), iterations=1)
    assert float((x[:, 30:40, 40:50] - 0.375).abs().max()) <= 8 * 2.0 ** -24


def black_rectangle_case():
    """the reflect case's blurred image with a black rectangle larger than the PSF's extent (42 columns x 27 rows) painted over it"""
    cs = case("reflect")
    y = cs["y16"].copy()
    y[:, 5:65, 10:80] = 0
    return cs, y


def check_black_rectangle(x, y):
    """wherever y == 0 the iteration keeps x == 0 (x_0 = y there and x only ever gets multiplied), all of it finite and in [0, 1]"""
    assert np.isfinite(x).all() and x.min() >= 0 and x.max() <= 1
    assert (x[y == 0] == 0).all() and (y == 0).sum() >= 3 * 60 * 70


def test_black_rectangle_stays_black_and_everything_is_finite():
    from detectinblur_amd.models import deconvolve as DC
    cs, y = black_rectangle_case()
    for n in (1, 5):
        check_black_rectangle(DC.richardson_lucy(torch.from_numpy(y.copy()), torch_psf(cs), iterations=n).numpy(), y)
    zeros = DC.richardson_lucy(torch.zeros(3, 70, 90, dtype=torch.float16), torch_psf(cs), iterations=3)      # y == 0 and A x == 0: q = 0
    assert torch.equal(zeros, torch.zeros(3, 70, 90))


def test_the_iteration_moves_toward_the_truth_and_the_data():
    from detectinblur_amd.models import deconvolve as DC
    cs = case("reflect")
    y = torch.from_numpy(cs["y16"].copy())
    y64 = cs["y16"].astype(np.float64)
    to_truth, to_data = [np.abs(y64 - cs["truth"]).mean()], [np.abs(ref_sweep(y64, cs["taps"], 128, False) - y64).mean()]
    for n in (5, 30):
        x = DC.richardson_lucy(y, torch_psf(cs), iterations=n).numpy().astype(np.float64)
        to_truth.append(np.abs(x - cs["truth"]).mean())
        to_data.append(np.abs(ref_sweep(x, cs["taps"], 128, False) - y64).mean())
    print("mean |x_N - truth| at N = 0, 5, 30:", to_truth, " mean |A x_N - y|:", to_data)
    assert to_truth[2] < to_truth[1] < to_truth[0] and to_data[2] < to_data[1] < to_data[0]


def test_python_argument_checks():
    from detectinblur_amd.models import deconvolve as DC
    cs = case("reflect")
    y = torch.from_numpy(cs["y16"].copy())
    for n in (0, 1001, -3):
        with pytest.raises(ValueError, match="iterations"):
            DC.richardson_lucy(y, torch_psf(cs), iterations=n)
        with pytest.raises(ValueError, match="iterations"):
            DC.Deconvolver(iterations=n)
    with pytest.raises(ValueError, match="eps"):
        DC.richardson_lucy(y, torch_psf(cs), eps=0.0)
    with pytest.raises(RuntimeError, match="Padding size"):
        DC.richardson_lucy(torch.zeros(3, 64, 90, dtype=torch.float16), torch_psf(cs), iterations=1)
    with pytest.raises(ValueError, match="128 x 128 or 256 x 256"):
        DC.richardson_lucy(y, torch.ones(64, 64), iterations=1)


# ---- 4: the C entry point ---------------------------------------------------------------------------------------------------------------

def test_entry_point_is_declared_and_bound():
    from detectinblur_amd import _lib
    header = open(os.path.join(ROOT, "include", "dib.h")).read()
    assert re.search(r"\bint dib_rl_deconvolve\(", header)
    assert "dib_rl_deconvolve" in _lib.EXPORTS and _lib.lib().dib_rl_deconvolve is not None
    assert _lib.lib().dib_abi_version() == 7
    assert "dib_deconv.hip" in open(os.path.join(ROOT, "detectinblur_amd", "csrc", "Makefile")).read()


def test_argument_errors_are_reported_without_a_gpu():
    """every refusal launches nothing and touches no pointer: the addresses below are never dereferenced"""
    from detectinblur_amd import _lib
    l = _lib.lib()
    y, out, work, tab = 1 << 20, 2 << 20, 3 << 20, 5 << 20

    def call(y=y, dtype=_lib.DIB_F16, out=out, work=work, C=3, H=70, W=90, tab=tab, psf_dtype=_lib.DIB_F16, K=128, n=5, eps=1e-6):
        return l.dib_rl_deconvolve(y, dtype, out, work, C, H, W, tab, psf_dtype, K, n, eps, None)
    E = _lib.DIB_EINVAL
    for kw in (dict(y=None), dict(out=None), dict(work=None), dict(tab=None)):
        assert call(**kw) == E and b"null pointer" in l.dib_last_error(), kw
    for n in (0, -1, 1001):
        assert call(n=n) == E and b"iterations" in l.dib_last_error(), n
    for kw in (dict(C=0), dict(H=0), dict(W=-2)):
        assert call(**kw) == E and b"empty shape" in l.dib_last_error(), kw
    for K in (64, 127, 129, 512):
        assert call(K=K) == E and b"K must be 128 or 256" in l.dib_last_error(), K
    for eps in (0.0, -1e-6, float("nan")):
        assert call(eps=eps) == E and b"eps" in l.dib_last_error(), eps
    assert call(dtype=2) == E and b"dtype" in l.dib_last_error()
    assert call(psf_dtype=5) == E and b"dtype" in l.dib_last_error()
    assert call(out=y) == E and b"overlap" in l.dib_last_error()
    assert call(work=out + 4) == E and b"overlap" in l.dib_last_error()
    # where the blur refuses the image (reflect padding of 63 / 64 on a side of 64)
    for kw in (dict(H=64), dict(W=64), dict(H=64, W=64)):
        assert call(**kw) == _lib.DIB_ESHAPE and b"Padding size" in l.dib_last_error(), kw
    assert call(H=64, W=1 << 14, C=1 << 15) == _lib.DIB_ESHAPE and b"too large" in l.dib_last_error()


# ---- 5: the driver ----------------------------------------------------------------------------------------------------------------------

def test_parser_defaults_and_train_does_not_know_the_flags():
    from detectinblur_amd import evaluate as EV, train as TR
    a = EV.build_parser().parse_args([])
    assert a.deconvolve_first is False and a.deconvolve_iterations == 30
    a = EV.build_parser().parse_args(["--deconvolve_first", "--deconvolve_iterations", "7"])
    assert a.deconvolve_first is True and a.deconvolve_iterations == 7
    helps = {s: act.help for act in EV.build_parser()._actions for s in act.option_strings}
    assert "(this repo)" in helps["--deconvolve_first"] and "--expand_target_boxes" in helps["--deconvolve_first"]
    assert "(this repo)" in helps["--deconvolve_iterations"]
    known = {s for act in TR.build_parser()._actions for s in act.option_strings}
    assert "--deconvolve_first" not in known and "--deconvolve_iterations" not in known
    with pytest.raises(SystemExit):
        quiet_err(TR.build_parser().parse_args, ["--deconvolve_first"])


def quiet_err(fn, *a):
    with contextlib.redirect_stderr(io.StringIO()):
        return fn(*a)


_ARGV = ["--synthetic", "--synthetic_images", "2", "--synthetic_size", "128", "160", "--min_size", "128", "--max_size", "160", "--device", "cpu",
         "--blur_eval", "--tensorboard_path", ""]


@pytest.mark.parametrize("extra,message", [
    (["--gpu_blur", "--deconvolve_first", "--deblur_first", "--deblurer_model_location", "X"], "--deconvolve_first with --deblur_first"),
    (["--deconvolve_first"], "--deconvolve_first needs --gpu_blur"),
    (["--deconvolve_first", "--cpu_blur"], "--deconvolve_first needs --gpu_blur"),
    (["--deconvolve_first", "--gpu_blur", "--cpu_blur"], "--deconvolve_first needs --gpu_blur"),
    (["--deconvolve_first", "--gpu_blur", "--vanilla_eval"], "--deconvolve_first with --vanilla_eval"),
    (["--gpu_blur", "--deconvolve_iterations", "30"], "--deconvolve_iterations needs --deconvolve_first"),
    (["--gpu_blur", "--deconvolve_first", "--deconvolve_iterations", "0"], "--deconvolve_iterations 0"),
    (["--gpu_blur", "--deconvolve_first", "--deconvolve_iterations", "1001"], "--deconvolve_iterations 1001"),
], ids=["deblur_first", "no_gpu_blur", "cpu_blur", "both_blurs", "vanilla", "idle_iterations", "zero", "too_many"])
def test_refusals_at_start(extra, message, monkeypatch):
    from detectinblur_amd import evaluate
    monkeypatch.setattr(evaluate, "fasterrcnn_resnet50_fpn", lambda *a, **k: pytest.fail("a detector was built"))
    with pytest.raises(SystemExit, match=re.escape(message)):
        evaluate.main(evaluate.build_parser().parse_args(_ARGV + extra))


def host_blur(images, blur_dicts, psfs_GPU=None, **kw):
    """stands in for --gpu_blur's launch on the host (the library has no CPU path): A of models/deconvolve.py, rounded to Half"""
    from detectinblur_amd.models import deconvolve as DC
    for i, bd in enumerate(blur_dicts):
        if bd["blurring"]:
            images[i] = DC.forward_blur(images[i], psfs_GPU[i]).half()


def test_evaluate_main_runs_a_cell_on_the_host(tmp_path, monkeypatch):
    from detectinblur_amd import evaluate as EV
    from detectinblur_amd.models import blur_functions as BF, deconvolve as DC
    from tests.test_engine_ddp_cpu import _small_model
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(EV, "SWEEP_PARAMS", EV.SWEEP_PARAMS[:1])
    monkeypatch.setattr(EV, "SWEEP_FRACTIONS", EV.SWEEP_FRACTIONS[2:3])
    monkeypatch.setattr(EV, "fasterrcnn_resnet50_fpn", lambda **kw: _small_model())
    monkeypatch.setattr(BF, "blur_image_list", host_blur)
    calls = []
    real = DC.Deconvolver.deconvolve_

    def counted(self, image, blur_dict, psf, tables=None, index=0):
        out = real(self, image, blur_dict, psf, tables, index)
        calls.append((self.iterations, bool(blur_dict["blurring"]), tuple(image.shape), image.dtype, tuple(out.shape), out.dtype, tables))
        return out
    monkeypatch.setattr(DC.Deconvolver, "deconvolve_", counted)
    args = EV.build_parser().parse_args(_ARGV + ["--gpu_blur", "--deconvolve_first", "--deconvolve_iterations", "2"])
    res = quiet(EV.main, args)
    assert len(res) == 1 and len(list(res.values())[0]["detections"]) == 2
    assert calls == [(2, True, (3, 128, 160), torch.float16, (3, 128, 160), torch.float32, None)] * 2


class Spy(object):
    """stands in for the Deconvolver: records what the engine hands it and what it hands back"""

    def __init__(self, real):
        self.real, self.inputs, self.outputs, self.dicts = real, [], [], []

    def deconvolve_(self, image, blur_dict, psf, tables=None, index=0):
        self.inputs.append(image.clone())
        self.dicts.append(blur_dict)
        out = self.real.deconvolve_(image, blur_dict, psf, tables, index)
        self.outputs.append(out.clone())
        return out


def blurring_loader(h, w, n, unblurred=()):
    """n synthetic images with a PSF each (blurred by the engine, not the loader); those listed in `unblurred` say blurring = False"""
    import random
    from tests.test_overlay import synthetic_loader
    np.random.seed(11)
    random.seed(11)
    loader = synthetic_loader(h, w, n=n, blur=True, blur_type=0.001, blur_ratio=1, blur_exposure=0.5)
    for i in unblurred:
        loader[i][2][0]["blurring"] = False
    return loader


def test_engine_hands_the_detector_the_deconvolved_image(monkeypatch):
    import copy
    from detectinblur_amd import engine
    from detectinblur_amd.models import blur_functions as BF, deconvolve as DC
    from tests.test_overlay import FixedDetector, fixed_detections
    monkeypatch.setattr(BF, "blur_image_list", host_blur)
    h, w, n = 70, 90, 3
    loader = blurring_loader(h, w, n, unblurred=(1,))
    cpu = torch.device("cpu")

    def run(**extra):
        model = FixedDetector(fixed_detections(h, w))
        quiet(engine.evaluate, model, type(loader)(copy.deepcopy(list(loader))), cpu, blurring_images=True, gpu_blur=True, **extra)
        return model.seen
    plain = run()
    real = DC.Deconvolver(iterations=3)
    spy = Spy(real)
    assert len(run(deconvolve_first=False, deconvolver=spy)) == n and spy.inputs == []
    seen = run(deconvolve_first=True, deconvolver=spy)
    assert len(seen) == n and len(spy.inputs) == 2 and all(d["blurring"] for d in spy.dicts)      # never for the image that was not blurred
    for k, i in enumerate((0, 2)):
        psf = torch.HalfTensor(loader[i][2][0]["psf"])
        assert spy.inputs[k].dtype == torch.float16 and torch.equal(spy.inputs[k].float(), plain[i])      # the blurred image, untouched
        assert seen[i].dtype == torch.float32 and torch.equal(seen[i], spy.outputs[k])
        assert torch.equal(seen[i], DC.richardson_lucy(spy.inputs[k], psf, iterations=3)) and not torch.equal(seen[i], plain[i])
    assert torch.equal(seen[1], plain[1])
    assert real.calls == 2
    # a pass that does not blur never runs the stage
    idle = Spy(real)
    model = FixedDetector(fixed_detections(h, w))
    quiet(engine.evaluate, model, type(loader)(copy.deepcopy(list(loader))), cpu, deconvolve_first=True, deconvolver=idle)
    assert idle.inputs == [] and len(model.seen) == n
    with pytest.raises(ValueError, match="deconvolver"):
        quiet(engine.evaluate, FixedDetector(fixed_detections(h, w)), loader, cpu, blurring_images=True, gpu_blur=True, deconvolve_first=True)
    with pytest.raises(ValueError, match="choose one"):
        quiet(engine.evaluate, FixedDetector(fixed_detections(h, w)), loader, cpu, blurring_images=True, gpu_blur=True, deconvolve_first=True,
              deconvolver=real, deblur_first=True, deblurer=object())
