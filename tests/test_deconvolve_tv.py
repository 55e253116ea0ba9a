"""`--deconvolve_tv` on the host: the total-variation factor and the regularised Richardson-Lucy iteration of models/deconvolve.py
(the torch restatement the drivers run under `--device cpu`) against the float64 statement of tests/_deconvolve_tv_cases.py, with its
tolerance rule; what the prior does (on the float64 reference first, then on the torch path); the argument checks of Python, of both C
entries and of the driver; and one sweep cell of evaluate.main with the flag.  tests/test_deconvolve_tv_gpu.py holds the HIP kernel
and stage to the same reference."""
import os
import re

import numpy as np
import pytest
import torch

from tests._deconvolve_tv_cases import (BETA, ITERATIONS, KERNEL_SHAPES, LAMBDAS, block_case, mse, plane_set, ref_rl_tv, reference_tv,
                                        reference_tv_weight, total_variation)
from tests.test_deconvolve_first import (_ARGV, EPS, HOST_CASES, ROOT, black_rectangle_case, case, check_black_rectangle, host_blur, quiet, ref_rl,
                                         torch_psf)


# ---- the definition -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("dtype", ["float16", "float32"])
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=["%dx%d" % s for s in KERNEL_SHAPES])
def test_tv_weight_torch_against_the_float64_definition(shape, dtype, lam):
    from detectinblur_amd.models import deconvolve as DC
    for C in (1, 3):
        x = plane_set(C, shape[0], shape[1], dtype)
        want, tol, d = reference_tv_weight(C, shape[0], shape[1], dtype, lam)
        got = DC.tv_weight_torch(torch.from_numpy(x.copy()), lam, BETA)
        assert got.dtype == torch.float32 and tuple(got.shape) == x.shape
        assert torch.equal(got, DC.tv_weight(torch.from_numpy(x.copy()), lam, BETA))      # a CPU tensor takes the restatement
        err = float(np.abs(got.numpy().astype(np.float64) - want).max())
        print("C=%d %s %s lambda=%g: torch vs float64 %.3g, float32 restatement %.3g, tolerance %.3g" % (C, shape, dtype, lam, err, d, tol))
        assert err <= tol, (C, err, tol)
    plane = torch.from_numpy(plane_set(1, shape[0], shape[1], dtype)[0].copy())      # H x W comes back H x W
    assert torch.equal(DC.tv_weight_torch(plane, lam, BETA), DC.tv_weight_torch(plane[None], lam, BETA)[0])


@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("iterations", ITERATIONS)
@pytest.mark.parametrize("name", HOST_CASES)
def test_torch_stage_against_the_float64_definition(name, iterations, lam):
    from detectinblur_amd.models import deconvolve as DC
    cs = case(name)
    want, tol, d = reference_tv(name, iterations, lam)
    got = DC.richardson_lucy(torch.from_numpy(cs["y16"].copy()), torch_psf(cs), iterations=iterations, eps=EPS, tv_lambda=lam, tv_beta=BETA)
    assert got.dtype == torch.float32 and tuple(got.shape) == cs["shape"] and not got.is_cuda
    err = float(np.abs(got.numpy().astype(np.float64) - want).max())
    print("%s N=%d lambda=%g: torch vs float64 %.3g, float32 restatement %.3g, tolerance %.3g" % (name, iterations, lam, err, d, tol))
    assert err <= tol, (err, tol)
    plain = ref_rl(cs["y16"], cs["taps"], cs["K"], iterations)
    assert float(np.abs(plain - want).max()) > 4 * tol      # the factor is not lost in the tolerance: plain RL fails this test


def test_without_the_prior_the_bits_are_the_plain_iterations():
    from detectinblur_amd.models import deconvolve as DC
    cs = case("reflect")
    y = torch.from_numpy(cs["y16"].copy())
    for n in (1, 4):
        plain = DC.richardson_lucy(y, torch_psf(cs), iterations=n)
        assert torch.equal(DC.richardson_lucy(y, torch_psf(cs), iterations=n, tv_lambda=0), plain)
        assert torch.equal(DC.richardson_lucy_torch(y, torch_psf(cs), n, 1e-6, 0.0, 1e-3), plain)
        assert not torch.equal(DC.richardson_lucy(y, torch_psf(cs), iterations=n, tv_lambda=0.002), plain)


# ---- behaviour ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", [0.0, 0.375, 1.0, 6.1e-5])
def test_a_constant_plane_comes_back_bit_for_bit(value):
    from detectinblur_amd.models import deconvolve as DC
    for dtype in (torch.float16, torch.float32):
        x = torch.full((3, 33, 65), value, dtype=dtype)
        for lam in LAMBDAS + (0.1,):
            assert torch.equal(DC.tv_weight_torch(x, lam, BETA), x.float())
    one = torch.tensor([[[0.7]]])
    assert torch.equal(DC.tv_weight_torch(one, 0.01, BETA), one)


def test_black_rectangle_stays_black_and_everything_is_finite():
    from detectinblur_amd.models import deconvolve as DC
    cs, y = black_rectangle_case()
    for n in (1, 5):
        check_black_rectangle(DC.richardson_lucy(torch.from_numpy(y.copy()), torch_psf(cs), iterations=n, tv_lambda=0.01).numpy(), y)
    w = DC.tv_weight_torch(torch.from_numpy(y.copy()), 0.01, BETA).numpy()
    assert np.isfinite(w).all() and (w[y == 0] == 0).all() and (w >= 0).all()
    zeros = DC.richardson_lucy(torch.zeros(3, 70, 90, dtype=torch.float16), torch_psf(cs), iterations=3, tv_lambda=0.01)
    assert torch.equal(zeros, torch.zeros(3, 70, 90))


def test_the_factor_is_positive_and_bounded():
    """|div| < 4: g lies in (1 / (1 + 4 lambda), 1 / (1 - 4 lambda)) whatever the image, also on the roughest one (a checkerboard of
    0 and 1) and at the largest lambda"""
    from detectinblur_amd.models import deconvolve as DC
    i, j = np.arange(33)[:, None], np.arange(65)[None, :]
    board = torch.from_numpy(((i + j) % 2).astype(np.float32))[None] * 0.5 + 0.25
    for lam in (0.002, 0.01, 0.1):
        g = DC.tv_weight_torch(board, lam, BETA) / board
        assert float(g.min()) > 1 / (1 + 4 * lam) - 1e-6 and float(g.max()) < 1 / (1 - 4 * lam) + 1e-6
        assert float(g.max()) > 1 and float(g.min()) < 1


def test_the_prior_lowers_the_error_and_the_total_variation_under_noise():
    """a piecewise-constant truth, blurred, with noise of sigma 0.03: at N = 30 and lambda = 0.01 the regularised iteration is closer to
    the truth than plain Richardson-Lucy and has a lower total variation -- on the float64 reference alone first (the property is the
    definition's), then on the torch path"""
    from detectinblur_amd.models import deconvolve as DC
    bc = block_case(0.03)
    n, lam = 30, 0.01
    plain = ref_rl(bc["y16"], bc["taps"], bc["K"], n)
    tv = ref_rl_tv(bc["y16"], bc["taps"], bc["K"], n, lam, BETA)
    figures = dict(mse_plain=mse(plain, bc["truth"]), mse_tv=mse(tv, bc["truth"]), tv_plain=total_variation(plain), tv_tv=total_variation(tv),
                   tv_truth=total_variation(bc["truth"]))
    print("float64:", figures)
    assert figures["mse_tv"] < figures["mse_plain"] and figures["tv_tv"] < figures["tv_plain"]
    y, psf = torch.from_numpy(bc["y16"].copy()), torch.from_numpy(bc["psf"].copy())
    t_plain = DC.richardson_lucy(y, psf, iterations=n).numpy()
    t_tv = DC.richardson_lucy(y, psf, iterations=n, tv_lambda=lam, tv_beta=BETA).numpy()
    print("torch: mse %.4g against %.4g, total variation %.5g against %.5g" % (mse(t_tv, bc["truth"]), mse(t_plain, bc["truth"]),
                                                                                total_variation(t_tv), total_variation(t_plain)))
    assert mse(t_tv, bc["truth"]) < mse(t_plain, bc["truth"]) and total_variation(t_tv) < total_variation(t_plain)


# ---- arguments ------------------------------------------------------------------------------------------------------------------------------

def test_python_argument_checks():
    from detectinblur_amd.models import deconvolve as DC
    cs = case("reflect")
    y = torch.from_numpy(cs["y16"].copy())
    for lam in (-0.01, 0.1000001, 0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tv_lambda"):
            DC.richardson_lucy(y, torch_psf(cs), iterations=1, tv_lambda=lam)
        with pytest.raises(ValueError, match="tv_lambda"):
            DC.Deconvolver(tv_lambda=lam)
        with pytest.raises(ValueError, match="tv_lambda"):
            DC.tv_weight_torch(y, lam)
    with pytest.raises(ValueError, match="tv_lambda"):
        DC.tv_weight_torch(y, 0.0)              # the factor itself has no "off"
    with pytest.raises(ValueError, match="tv_lambda"):
        DC.tv_weight(y, 0.0)
    for beta in (0.0, -1e-2, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tv_beta"):
            DC.richardson_lucy(y, torch_psf(cs), iterations=1, tv_lambda=0.01, tv_beta=beta)
        with pytest.raises(ValueError, match="tv_beta"):
            DC.Deconvolver(tv_lambda=0.01, tv_beta=beta)
        with pytest.raises(ValueError, match="tv_beta"):
            DC.tv_weight_torch(y, 0.01, beta)
    d = DC.Deconvolver()
    assert d.tv_lambda == 0.0 and d.tv_beta == 1e-2 and DC.DEFAULT_TV_BETA == 1e-2
    d = DC.Deconvolver(iterations=3, tv_lambda=0.1, tv_beta=0.5)
    assert (d.iterations, d.tv_lambda, d.tv_beta) == (3, 0.1, 0.5)
    with pytest.raises(ValueError, match="C x H x W"):
        DC.tv_weight_torch(torch.zeros(2, 3, 4, 5), 0.01)


def test_entry_points_are_declared_and_bound():
    from detectinblur_amd import _lib
    header = open(os.path.join(ROOT, "include", "dib.h")).read()
    for name in ("dib_tv_weight", "dib_rl_deconvolve_tv"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTS and getattr(_lib.lib(), name) is not None
    assert re.search(r"\bint dib_rl_deconvolve\(const void \*y_dev, int dtype, float \*out_dev, float \*work_dev, int C, int H, int W, "
                     r"const void \*table_dev,\s+int psf_dtype, int K, int iterations, float eps, void \*stream\);", header)
    assert _lib.lib().dib_abi_version() == 7
    assert "dib_deconv_tv.hip" in open(os.path.join(ROOT, "detectinblur_amd", "csrc", "Makefile")).read()


def test_argument_errors_of_the_factor_are_reported_without_a_gpu():
    """every refusal launches nothing and touches no pointer: the addresses below are never dereferenced"""
    from detectinblur_amd import _lib
    l = _lib.lib()
    x, out = 1 << 20, 2 << 20

    def call(x=x, dtype=_lib.DIB_F16, out=out, C=3, H=70, W=90, lam=0.01, beta=1e-2):
        return l.dib_tv_weight(x, dtype, out, C, H, W, lam, beta, None)
    E = _lib.DIB_EINVAL
    for kw in (dict(x=None), dict(out=None)):
        assert call(**kw) == E and b"null pointer" in l.dib_last_error(), kw
    for dtype in (2, -1, 7):
        assert call(dtype=dtype) == E and b"dtype" in l.dib_last_error(), dtype
    for kw in (dict(C=0), dict(H=0), dict(W=-2)):
        assert call(**kw) == E and b"empty shape" in l.dib_last_error(), kw
    for lam in (0.0, -0.01, 0.11, float("nan"), float("inf")):
        assert call(lam=lam) == E and b"tv_lambda" in l.dib_last_error(), lam
    for beta in (0.0, -1e-2, float("nan"), float("inf")):
        assert call(beta=beta) == E and b"tv_beta" in l.dib_last_error(), beta
    assert call(out=x) == E and b"overlap" in l.dib_last_error()
    assert call(out=x + 3 * 70 * 90 * 2 - 2) == E and b"overlap" in l.dib_last_error()      # the Half input's last element
    assert call(x=out + 3 * 70 * 90 * 4 - 4, dtype=_lib.DIB_F32) == E and b"overlap" in l.dib_last_error()
    assert call(H=1 << 15, W=1 << 15, C=2) == _lib.DIB_ESHAPE and b"too large" in l.dib_last_error()
    assert call(H=1, W=1, C=(1 << 31) - 1) == _lib.DIB_ESHAPE and b"too large" in l.dib_last_error()


def test_argument_errors_of_the_stage_are_reported_without_a_gpu():
    from detectinblur_amd import _lib
    l = _lib.lib()
    y, out, work, tab = 1 << 20, 2 << 20, 3 << 20, 5 << 20
    n = 3 * 70 * 90

    def call(y=y, dtype=_lib.DIB_F16, out=out, work=work, C=3, H=70, W=90, tab=tab, psf_dtype=_lib.DIB_F16, K=128, n=5, eps=1e-6, lam=0.01, beta=1e-2):
        return l.dib_rl_deconvolve_tv(y, dtype, out, work, C, H, W, tab, psf_dtype, K, n, eps, lam, beta, None)
    E = _lib.DIB_EINVAL
    for kw in (dict(y=None), dict(out=None), dict(work=None), dict(tab=None)):
        assert call(**kw) == E and b"null pointer" in l.dib_last_error(), kw
    for it in (0, -1, 1001):
        assert call(n=it) == E and b"iterations" in l.dib_last_error(), it
    for kw in (dict(C=0), dict(H=0), dict(W=-2)):
        assert call(**kw) == E and b"empty shape" in l.dib_last_error(), kw
    for K in (64, 127, 129, 512):
        assert call(K=K) == E and b"K must be 128 or 256" in l.dib_last_error(), K
    for eps in (0.0, -1e-6, float("nan")):
        assert call(eps=eps) == E and b"eps" in l.dib_last_error(), eps
    assert call(dtype=2) == E and b"dtype" in l.dib_last_error()
    assert call(psf_dtype=5) == E and b"dtype" in l.dib_last_error()
    for lam in (0.0, -0.01, 0.11, float("nan")):
        assert call(lam=lam) == E and b"tv_lambda" in l.dib_last_error(), lam
    for beta in (0.0, -1e-2, float("nan"), float("inf")):
        assert call(beta=beta) == E and b"tv_beta" in l.dib_last_error(), beta
    assert call(out=y) == E and b"overlap" in l.dib_last_error()
    assert call(work=out + 4) == E and b"overlap" in l.dib_last_error()
    # the workspace is three planes: an output inside its third plane is refused here, and accepted by the plain entry's two planes
    assert call(out=work + 2 * n * 4) == E and b"overlap" in l.dib_last_error()
    assert call(out=work + 3 * n * 4, n=0) == E and b"iterations" in l.dib_last_error()      # (past the third plane: not an overlap)
    for kw in (dict(H=64), dict(W=64), dict(H=64, W=64)):
        assert call(**kw) == _lib.DIB_ESHAPE and b"Padding size" in l.dib_last_error(), kw
    assert call(H=64, W=1 << 14, C=1 << 15) == _lib.DIB_ESHAPE and b"too large" in l.dib_last_error()
    assert b"dib_rl_deconvolve_tv" in l.dib_last_error()


# ---- the driver -----------------------------------------------------------------------------------------------------------------------------

def test_parser_default_and_help_and_train_does_not_know_the_flag():
    from detectinblur_amd import evaluate as EV, train as TR
    assert EV.build_parser().parse_args([]).deconvolve_tv is None
    a = EV.build_parser().parse_args(["--deconvolve_first", "--deconvolve_tv", "0.005"])
    assert a.deconvolve_first is True and a.deconvolve_tv == 0.005
    text = {s: act.help for act in EV.build_parser()._actions for s in act.option_strings}["--deconvolve_tv"]
    assert "(this repo)" in text and "0.002 to 0.01" in text and "flatten detail" in text
    assert "--deconvolve_tv" not in {s for act in TR.build_parser()._actions for s in act.option_strings}
    d = EV.build_deconvolver(a)
    assert (d.tv_lambda, d.tv_beta, d.iterations) == (0.005, 1e-2, 30)
    d = EV.build_deconvolver(EV.build_parser().parse_args(["--deconvolve_first"]))
    assert (d.tv_lambda, d.tv_beta) == (0.0, 1e-2)
    assert EV.build_deconvolver(EV.build_parser().parse_args([])) is None


@pytest.mark.parametrize("extra,message", [
    (["--gpu_blur", "--deconvolve_tv", "0.01"], "--deconvolve_tv needs --deconvolve_first"),
    (["--gpu_blur", "--deconvolve_first", "--deconvolve_tv", "0"], "--deconvolve_tv 0"),
    (["--gpu_blur", "--deconvolve_first", "--deconvolve_tv", "-0.01"], "--deconvolve_tv -0.01"),
    (["--gpu_blur", "--deconvolve_first", "--deconvolve_tv", "0.2"], "--deconvolve_tv 0.2"),
    (["--gpu_blur", "--deconvolve_first", "--deconvolve_tv", "nan"], "--deconvolve_tv nan"),
    (["--deconvolve_first", "--deconvolve_tv", "0.01"], "--deconvolve_first needs --gpu_blur"),
], ids=["no_stage", "zero", "negative", "too_large", "nan", "no_gpu_blur"])
def test_refusals_at_start(extra, message, monkeypatch):
    from detectinblur_amd import evaluate
    monkeypatch.setattr(evaluate, "fasterrcnn_resnet50_fpn", lambda *a, **k: pytest.fail("a detector was built"))
    with pytest.raises(SystemExit, match=re.escape(message)):
        evaluate.main(evaluate.build_parser().parse_args(_ARGV + extra))


def test_evaluate_main_runs_a_cell_on_the_host_and_the_detector_gets_the_regularised_image(tmp_path, monkeypatch):
    from detectinblur_amd import evaluate as EV
    from detectinblur_amd.models import blur_functions as BF, deconvolve as DC
    from tests.test_engine_ddp_cpu import _small_model
    monkeypatch.chdir(tmp_path)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(EV, "SWEEP_PARAMS", EV.SWEEP_PARAMS[:1])
    monkeypatch.setattr(EV, "SWEEP_FRACTIONS", EV.SWEEP_FRACTIONS[2:3])
    seen = []

    def watched(**kw):
        model = _small_model()
        model.register_forward_pre_hook(lambda module, args: seen.append(args[0][0].detach().clone()))
        return model
    monkeypatch.setattr(EV, "fasterrcnn_resnet50_fpn", watched)
    monkeypatch.setattr(BF, "blur_image_list", host_blur)
    calls = []
    real = DC.Deconvolver.deconvolve_

    def counted(self, image, blur_dict, psf, tables=None, index=0):
        out = real(self, image, blur_dict, psf, tables, index)
        calls.append((self.iterations, self.tv_lambda, self.tv_beta, image.clone(), psf.clone(), out.clone()))
        return out
    monkeypatch.setattr(DC.Deconvolver, "deconvolve_", counted)
    args = EV.build_parser().parse_args(_ARGV + ["--gpu_blur", "--deconvolve_first", "--deconvolve_iterations", "2", "--deconvolve_tv", "0.01"])
    res = quiet(EV.main, args)
    assert len(res) == 1 and len(list(res.values())[0]["detections"]) == 2
    assert len(calls) == 2 and len(seen) == 2
    for (n, lam, beta, image, psf, out), got in zip(calls, seen):
        assert (n, lam, beta) == (2, 0.01, 1e-2) and image.dtype == torch.float16 and tuple(image.shape) == (3, 128, 160)
        want = DC.richardson_lucy_torch(image, psf, iterations=2, tv_lambda=0.01, tv_beta=1e-2)
        assert out.dtype == torch.float32 and torch.equal(out, want) and torch.equal(got, want)
        assert not torch.equal(want, DC.richardson_lucy_torch(image, psf, iterations=2))
