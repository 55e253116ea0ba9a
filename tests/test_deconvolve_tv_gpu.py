"""`--deconvolve_tv` on the GPU: the kernel of csrc/dib_deconv_tv.hip (dib_tv_weight) and the regularised stage (dib_rl_deconvolve_tv)
against the float64 statement of tests/_deconvolve_tv_cases.py, with its tolerance rule max(8 d, N 2^-20), d <= 2^-12 asserted; the
planes of one image kept apart; nothing written or read beyond the buffers; agreement with the torch restatement on the same device;
determinism, graph capture, odd and even counts; the plain stage untouched; and engine.evaluate handing the detector the regularised
image."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests._deconvolve_tv_cases import BETA, ITERATIONS, KERNEL_SHAPES, LAMBDAS, image_np, plane_set, reference_tv, reference_tv_weight
from tests.test_deconvolve_first import EPS, Spy, black_rectangle_case, blurring_loader, case, check_black_rectangle

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
STAGE_CASES = ("reflect", "reflect65", "zero", "replicate", "oneplane")
GUARD = 4096      # elements of NaN on either side of a guarded buffer


def tables_of(cs):
    from detectinblur_amd import blur_ops
    return blur_ops.compact_psfs([torch.from_numpy(cs["psf"].copy()).to(DEV)], normalize=True)


def guarded(n, dtype=torch.float32):
    """(the whole buffer, the n elements in its middle): NaN all over"""
    whole = torch.full((GUARD + n + GUARD,), float("nan"), dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n]


def guards_are_untouched(whole):
    return bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[-GUARD:]).all())


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["float16", "float32"])
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=["%dx%d" % s for s in KERNEL_SHAPES])
def test_tv_weight_against_the_float64_definition(shape, dtype):
    """planes at 0.1 / 0.9 / 0.5: a stencil that crosses from one plane into the next, or from a row's end into the next row, is off
    by far more than the tolerance.  The input sits between NaN guard bands, as does the output: a read beyond the input poisons the
    result, a write beyond the output shows in its band"""
    from detectinblur_amd import _lib
    from detectinblur_amd.models import deconvolve as DC
    H, W = shape
    for C in (1, 3):
        x = plane_set(C, H, W, dtype)
        x_whole, x_dev = guarded(C * H * W, getattr(torch, dtype))
        x_dev.copy_(torch.from_numpy(x.copy()).reshape(-1))
        for lam in LAMBDAS:
            want, tol, d = reference_tv_weight(C, H, W, dtype, lam)
            out_whole, out = guarded(C * H * W)
            _lib.check(_lib.lib().dib_tv_weight(x_dev.data_ptr(), _lib.DIB_F16 if dtype == "float16" else _lib.DIB_F32, out.data_ptr(), C, H, W,
                                                lam, BETA, _lib.stream_of(x_dev)))
            torch.cuda.synchronize()
            assert guards_are_untouched(out_whole) and guards_are_untouched(x_whole)
            got = out.cpu().numpy().astype(np.float64).reshape(C, H, W)
            assert np.isfinite(got).all()
            err = float(np.abs(got - want).max())
            print("C=%d %s %s lambda=%g: HIP vs float64 %.3g, float32 restatement %.3g, tolerance %.3g" % (C, shape, dtype, lam, err, d, tol))
            assert err <= tol, (C, lam, err, tol)
            via_python = DC.tv_weight(x_dev.reshape(C, H, W), lam, BETA)
            assert via_python.dtype == torch.float32 and tuple(via_python.shape) == (C, H, W) and torch.equal(via_python.reshape(-1), out)
            ref = DC.tv_weight_torch(x_dev.reshape(C, H, W), lam, BETA)
            assert ref.is_cuda and float((via_python - ref).abs().max()) <= tol


def test_constants_and_black_come_back_bit_for_bit():
    from detectinblur_amd.models import deconvolve as DC
    for dtype in (torch.float16, torch.float32):
        for value in (0.0, 0.375, 1.0):
            x = torch.full((3, 33, 65), value, dtype=dtype, device=DEV)
            assert torch.equal(DC.tv_weight(x, 0.01, BETA), x.float())
    one = torch.tensor([[[0.7]]], device=DEV)
    assert torch.equal(DC.tv_weight(one, 0.01, BETA), one)
    cs, y = black_rectangle_case()
    tables = tables_of(cs)
    for n in (1, 5):
        check_black_rectangle(DC.richardson_lucy(torch.from_numpy(y.copy()).to(DEV), tables, iterations=n, tv_lambda=0.01).cpu().numpy(), y)


# ---- the stage ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("y_dtype", ["float16", "float32"])
@pytest.mark.parametrize("name", STAGE_CASES)
def test_stage_against_the_float64_definition(name, y_dtype):
    from detectinblur_amd.models import deconvolve as DC
    cs = case(name)
    tables = tables_of(cs)
    y = torch.from_numpy(image_np(name, y_dtype).copy()).to(DEV)
    for lam in LAMBDAS:
        for n in ITERATIONS:
            want, tol, d = reference_tv(name, n, lam, y_dtype)
            got = DC.richardson_lucy(y, tables, iterations=n, eps=EPS, tv_lambda=lam, tv_beta=BETA)
            assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == cs["shape"]
            err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
            print("%s %s N=%d lambda=%g: HIP vs float64 %.3g, float32 restatement %.3g, tolerance %.3g" % (name, y_dtype, n, lam, err, d, tol))
            assert err <= tol, (lam, n, err, tol)


@pytest.mark.parametrize("name", ["reflect", "zero", "replicate"])
def test_stage_against_the_torch_path_on_the_gpu_and_itself(name):
    from detectinblur_amd.models import deconvolve as DC
    cs = case(name)
    tables = tables_of(cs)
    y = torch.from_numpy(cs["y16"].copy()).to(DEV)
    taps = DC.taps_of_table(tables, 0)
    lam = 0.01
    for n in (2, 5):
        _, tol, _ = reference_tv(name, n, lam)
        hip = DC.richardson_lucy(y, tables, iterations=n, eps=EPS, tv_lambda=lam, tv_beta=BETA)
        ref = DC.richardson_lucy_torch(y, taps, iterations=n, eps=EPS, tv_lambda=lam, tv_beta=BETA)
        assert ref.is_cuda and float((hip - ref).abs().max()) <= tol
        assert torch.equal(hip, DC.richardson_lucy(y, tables, iterations=n, eps=EPS, tv_lambda=lam, tv_beta=BETA))                # deterministic
        assert torch.equal(hip, DC.richardson_lucy(y, torch.from_numpy(cs["psf"].copy()), iterations=n, eps=EPS, tv_lambda=lam, tv_beta=BETA))
        assert not torch.equal(hip, DC.richardson_lucy(y, tables, iterations=n, eps=EPS))
    # captured into a graph and replayed: the same bits (no allocation, no synchronisation, no library state in the call)
    eager = DC.richardson_lucy_hip(y, tables, 0, 5, EPS, lam, BETA)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        DC.richardson_lucy_hip(y, tables, 0, 5, EPS, lam, BETA)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = DC.richardson_lucy_hip(y, tables, 0, 5, EPS, lam, BETA)
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)


@pytest.mark.parametrize("y_dtype", ["float16", "float32"])
def test_odd_and_even_counts_end_in_out_and_stay_inside_the_buffers(y_dtype):
    """the C entry itself, every buffer between NaN guard bands: the result is in out_dev for N = 4 and N = 5, it is what the Python
    entry returns, nothing beyond the three workspace planes, the output or the input is written, and a read beyond the input would
    poison the result"""
    from detectinblur_amd import _lib
    from detectinblur_amd.models import deconvolve as DC
    cs = case("reflect")
    C, H, W = cs["shape"]
    n = C * H * W
    tables = tables_of(cs)
    y_whole, y = guarded(n, getattr(torch, y_dtype))
    y.copy_(torch.from_numpy(image_np("reflect", y_dtype).copy()).reshape(-1))
    for count in (4, 5):
        out_whole, out = guarded(n)
        work_whole, work = guarded(3 * n)
        _lib.check(_lib.lib().dib_rl_deconvolve_tv(y.data_ptr(), _lib.DIB_F16 if y_dtype == "float16" else _lib.DIB_F32, out.data_ptr(),
                                                   work.data_ptr(), C, H, W, tables.ptr(0), _lib.DIB_F16, cs["K"], count, EPS, 0.01, BETA,
                                                   _lib.stream_of(y)))
        torch.cuda.synchronize()
        assert guards_are_untouched(out_whole) and guards_are_untouched(work_whole) and guards_are_untouched(y_whole)
        want, tol, _ = reference_tv("reflect", count, 0.01, y_dtype)
        assert float(np.abs(out.cpu().numpy().astype(np.float64).reshape(C, H, W) - want).max()) <= tol
        assert torch.equal(out.reshape(C, H, W), DC.richardson_lucy(y.reshape(C, H, W), tables, iterations=count, eps=EPS, tv_lambda=0.01, tv_beta=BETA))


def test_the_plain_stage_is_the_plain_entry():
    """richardson_lucy without the argument (and with tv_lambda = 0) = dib_rl_deconvolve called directly, bit for bit, with its
    two-plane workspace"""
    from detectinblur_amd import _lib
    from detectinblur_amd.models import deconvolve as DC
    cs = case("reflect")
    C, H, W = cs["shape"]
    tables = tables_of(cs)
    y = torch.from_numpy(cs["y16"].copy()).to(DEV)
    for count in (1, 4):
        out_whole, out = guarded(C * H * W)
        work_whole, work = guarded(2 * C * H * W)
        _lib.check(_lib.lib().dib_rl_deconvolve(y.data_ptr(), _lib.DIB_F16, out.data_ptr(), work.data_ptr(), C, H, W, tables.ptr(0), _lib.DIB_F16,
                                                cs["K"], count, EPS, _lib.stream_of(y)))
        torch.cuda.synchronize()
        assert guards_are_untouched(out_whole) and guards_are_untouched(work_whole)
        assert torch.equal(DC.richardson_lucy(y, tables, iterations=count, eps=EPS).reshape(-1), out)
        assert torch.equal(DC.richardson_lucy(y, tables, iterations=count, eps=EPS, tv_lambda=0.0).reshape(-1), out)


# ---- the engine -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loop", ["pipelined", "no_graphs"])
def test_engine_hands_the_detector_the_regularised_image(monkeypatch, loop):
    from detectinblur_amd import engine
    from detectinblur_amd.models import deconvolve as DC
    from tests.test_overlay import fixed_detections
    from tests.test_overlay_gpu import SplitDetector
    monkeypatch.delenv("DIB_NO_PIPELINE", raising=False)
    if loop == "no_graphs":
        monkeypatch.setenv("DIB_NO_GRAPHS", "1")
    else:
        monkeypatch.delenv("DIB_NO_GRAPHS", raising=False)
    h, w, n = 128, 160, 3
    dets = fixed_detections(h, w)
    loader = blurring_loader(h, w, n, unblurred=(1,))

    def run(**kw):
        model = SplitDetector(dets)
        with contextlib.redirect_stdout(io.StringIO()):
            engine.evaluate(None, loader, DEV, blurring_images=True, gpu_blur=True, expand_target_boxes=True, use_ensemble=True,
                            ensemble_models=[model] * 4, **kw)
        return model.seen
    blurred = run()
    spy = Spy(DC.Deconvolver(iterations=4, tv_lambda=0.01))
    seen = run(deconvolve_first=True, deconvolver=spy)
    assert len(seen) == n and len(spy.inputs) == 2
    for k, i in enumerate((0, 2)):
        psf = torch.HalfTensor(loader[i][2][0]["psf"]).to(DEV)
        assert spy.inputs[k].dtype == torch.float16 and torch.equal(spy.inputs[k].float(), blurred[i].float())      # the blurred image
        assert seen[i].dtype == torch.float32 and seen[i].is_cuda and torch.equal(seen[i], spy.outputs[k])
        assert torch.equal(seen[i], DC.richardson_lucy(spy.inputs[k], psf, iterations=4, tv_lambda=0.01, tv_beta=1e-2))
        assert not torch.equal(seen[i], DC.richardson_lucy(spy.inputs[k], psf, iterations=4))
    assert torch.equal(seen[1].float(), blurred[1].float())
