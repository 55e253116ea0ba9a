"""`--deconvolve_first` on the GPU: the two sweep kernels of csrc/dib_deconv.hip (dib_rl_deconvolve) against the float64 definition of
tests/test_deconvolve_first.py -- same cases, same tolerance rule max(8 d, N 2^-20) with d the float32 restatement's own deviation --
and against the torch restatement on the same device; determinism, graph capture, the black rectangle; and engine.evaluate handing the
detector the deconvolved image in the graphed / pipelined loop and in the plain one."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests.test_deconvolve_first import (EPS, ITERATIONS, Spy, black_rectangle_case, blurring_loader, case, check_black_rectangle, ref_sweep,
                                         reference)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
_NP = {"float16": np.float16, "float32": np.float32}


def tables_of(cs, **kw):
    from detectinblur_amd import blur_ops
    return blur_ops.compact_psfs([torch.from_numpy(cs["psf"].copy()).to(DEV)], normalize=True, **kw)


def image_of(cs, y_dtype):
    """the case's blurred image on the device: the Half one, or the fp32 rounding of the same float64 blur (as reference() builds it)"""
    if y_dtype == "float16":
        return torch.from_numpy(cs["y16"].copy()).to(DEV)
    return torch.from_numpy(ref_sweep(cs["truth"], cs["taps"], cs["K"], False).astype(np.float32)).to(DEV)


# (case, image dtype, PSF dtype): every case with the drivers' types (Half image, Half PSF); fp32 images and fp32 PSF tables on one case
# of each canvas
COMBOS = [(name, "float16", "float16") for name in ("reflect", "reflect65", "zero", "replicate", "oneplane", "dense")] + \
         [("reflect", "float32", "float16"), ("reflect", "float16", "float32"), ("replicate", "float32", "float32")]


@pytest.mark.parametrize("iterations", ITERATIONS)
@pytest.mark.parametrize("name,y_dtype,psf_dtype", COMBOS, ids=["-".join(c) for c in COMBOS])
def test_hip_against_the_float64_definition(name, y_dtype, psf_dtype, iterations):
    from detectinblur_amd.models import deconvolve as DC
    cs = case(name, psf_dtype)
    want, tol, d = reference(name, iterations, y_dtype, psf_dtype)
    tables = tables_of(cs)
    assert tables.dtype == getattr(torch, psf_dtype)
    if name == "dense":
        assert tables.header(0)[0] > 1000 and len(tables.segments(0)) > 50
    got = DC.richardson_lucy(image_of(cs, y_dtype), tables, iterations=iterations, eps=EPS)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == cs["shape"]
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print("%s %s/%s N=%d: HIP vs float64 %.3g, float32 restatement %.3g, tolerance %.3g" % (name, y_dtype, psf_dtype, iterations, err, d, tol))
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("flags", [dict(large_window=True), dict(vruns=True)], ids=["large_window", "vruns"])
def test_tables_of_the_other_geometries_are_served(flags):
    """a table compacted for the large LDS window (boxes of up to 21 x 64) is cut into windows of 13 x 25 by the kernel: another tap
    order, the same tolerance; one that carries the vertical-run groups has the same tap list: the same bits"""
    from detectinblur_amd.models import deconvolve as DC
    cs = case("reflect")
    want, tol, _ = reference("reflect", 5)
    y = image_of(cs, "float16")
    got = DC.richardson_lucy(y, tables_of(cs, **flags), iterations=5, eps=EPS)
    assert float(np.abs(got.cpu().numpy().astype(np.float64) - want).max()) <= tol
    if "vruns" in flags:
        assert torch.equal(got, DC.richardson_lucy(y, tables_of(cs), iterations=5, eps=EPS))


@pytest.mark.parametrize("name", ["reflect", "zero", "replicate"])
def test_hip_against_the_torch_path_on_the_gpu_and_itself(name):
    from detectinblur_amd.models import deconvolve as DC
    cs = case(name)
    tables, y = tables_of(cs), image_of(cs, "float16")
    taps = DC.taps_of_table(tables, 0)
    assert np.array_equal(taps.rows.numpy(), cs["taps"][0]) and np.array_equal(taps.weights.numpy().astype(np.float64), cs["taps"][2])
    for n in (2, 5):
        _, tol, _ = reference(name, n)
        hip = DC.richardson_lucy(y, tables, iterations=n, eps=EPS)
        ref = DC.richardson_lucy_torch(y, taps, iterations=n, eps=EPS)
        assert ref.is_cuda and float((hip - ref).abs().max()) <= tol
        assert torch.equal(hip, DC.richardson_lucy(y, tables, iterations=n, eps=EPS))                # deterministic
        assert torch.equal(hip, DC.richardson_lucy(y, torch.from_numpy(cs["psf"].copy()), iterations=n, eps=EPS))      # from the PSF itself
    # captured into a graph and replayed: the same bits (no allocation, no synchronisation, no library state in the call)
    eager = DC.richardson_lucy_hip(y, tables, 0, 5, EPS)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        DC.richardson_lucy_hip(y, tables, 0, 5, EPS)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = DC.richardson_lucy_hip(y, tables, 0, 5, EPS)
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)


def test_black_rectangle_stays_black_and_everything_is_finite():
    from detectinblur_amd.models import deconvolve as DC
    cs, y = black_rectangle_case()
    tables = tables_of(cs)
    for n in (1, 5):
        check_black_rectangle(DC.richardson_lucy(torch.from_numpy(y.copy()).to(DEV), tables, iterations=n).cpu().numpy(), y)
    zeros = DC.richardson_lucy(torch.zeros(3, 70, 90, dtype=torch.float16, device=DEV), tables, iterations=3)
    assert torch.equal(zeros, torch.zeros(3, 70, 90, device=DEV))


@pytest.mark.parametrize("loop", ["pipelined", "no_graphs"])
def test_engine_hands_the_detector_the_deconvolved_image(tmp_path, monkeypatch, loop):
    """after --gpu_blur and the box growth, in the look-ahead: the detector and the picture get richardson_lucy of the blurred Half image,
    fp32, the image that was not blurred stays as it was, the detections are those of the run without the stage, and the loop
    synchronises no more often than without it"""
    from detectinblur_amd import engine, overlay
    from detectinblur_amd.models import deconvolve as DC
    from tests.test_overlay import fixed_detections, read_png
    from tests.test_overlay_gpu import SplitDetector
    monkeypatch.delenv("DIB_NO_PIPELINE", raising=False)
    if loop == "no_graphs":
        monkeypatch.setenv("DIB_NO_GRAPHS", "1")
    else:
        monkeypatch.delenv("DIB_NO_GRAPHS", raising=False)
    h, w, n = 70, 101, 3
    dets = fixed_detections(h, w)
    loader = blurring_loader(h, w, n, unblurred=(1,))
    syncs = [0]
    real_sync = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: syncs.__setitem__(0, syncs[0] + 1) or real_sync(*a, **k))

    def run(folder=None, **kw):
        model = SplitDetector(dets)
        syncs[0] = 0
        with contextlib.redirect_stdout(io.StringIO()):
            res = engine.evaluate(None, loader, DEV, blurring_images=True, gpu_blur=True, expand_target_boxes=True, use_ensemble=True,
                                  ensemble_models=[model] * 4, image_output_folder=folder, **kw)
        return model.seen, syncs[0], res["detections"]
    blurred, syncs_plain, dets_plain = run()
    real = DC.Deconvolver(iterations=4)
    spy = Spy(real)
    seen, syncs_stage, dets_stage = run(folder=str(tmp_path / "pics"), deconvolve_first=True, deconvolver=spy)
    assert syncs_stage == syncs_plain and len(seen) == n and len(spy.inputs) == 2
    assert sorted(dets_stage) == sorted(dets_plain)
    for k in dets_plain:
        assert all(torch.equal(dets_stage[k][f], dets_plain[k][f]) for f in dets_plain[k])
    for k, i in enumerate((0, 2)):
        psf = torch.HalfTensor(loader[i][2][0]["psf"]).to(DEV)
        assert spy.inputs[k].dtype == torch.float16 and torch.equal(spy.inputs[k].float(), blurred[i].float())      # the blurred image
        assert seen[i].dtype == torch.float32 and seen[i].is_cuda and torch.equal(seen[i], spy.outputs[k])
        assert torch.equal(seen[i], DC.richardson_lucy(spy.inputs[k], psf, iterations=4)) and not torch.equal(seen[i], blurred[i].float())
    assert torch.equal(seen[1].float(), blurred[1].float())
    for i in range(n):
        want = overlay.render_host(seen[i].cpu(), dets[i]["boxes"], dets[i]["labels"], dets[i]["scores"])
        assert np.array_equal(read_png(tmp_path / "pics" / ("img%d.png" % i)), want), i
