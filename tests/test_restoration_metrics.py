"""`--restoration_metrics` on the host: quality.restoration_quality's torch path against the float64 definition of tests/test_quality.py
(the same cases, the same tolerance rule), the 8-bit form against that definition on numpy-quantised images with L = 255, the
accumulator's semantics, the C entry's argument checks, evaluate.py's refusals, and the meter inside engine.evaluate on the CPU.
tests/test_restoration_metrics_gpu.py holds the HIP kernel to the single-pair kernel bit for bit."""
import contextlib
import copy
import ctypes
import io
import math
import re

import numpy as np
import pytest
import torch

from tests.test_quality import KINDS, PSNR_TOL, SHAPES, SSIM_CAP, case, check_against_reference, ref_quality, ref_quality_tiled


def tensors(cs):
    return torch.from_numpy(cs["a"].copy()), torch.from_numpy(cs["b"].copy())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_torch_path_against_the_float64_definition(shape, kind):
    from detectinblur_amd import quality as Q
    cs0, cs1 = case(kind, shape, "float16", "float32"), case(kind, shape, "float32", "float32")
    (a0, ref), (a1, ref1) = tensors(cs0), tensors(cs1)
    assert torch.equal(ref, ref1)
    one = Q.restoration_quality(ref, a0)
    assert one.dtype == torch.float32 and tuple(one.shape) == (3,) and not one.is_cuda
    check_against_reference(one.tolist(), cs0, "torch K = 1 %s %s" % (kind, shape))
    two = Q.restoration_quality(ref, [a1, a0])
    assert tuple(two.shape) == (6,)
    check_against_reference(two[:3].tolist(), cs1, "torch K = 2 slot 0 %s %s" % (kind, shape))
    check_against_reference(two[3:].tolist(), cs0, "torch K = 2 slot 1 %s %s" % (kind, shape))
    assert torch.equal(two[3:], Q.psnr_ssim(a0, ref)) and torch.equal(two[:3], Q.psnr_ssim(a1, ref))


def np_grey8(x):
    return np.rint(np.clip(np.asarray(x, dtype=np.float32) * np.float32(255), 0, 255)).astype(np.float32)


def test_quantize8_against_the_definition_on_quantised_images():
    from detectinblur_amd import quality as Q
    rng = np.random.RandomState(4)
    shape = (3, 37, 53)
    ref, cand = rng.uniform(0, 1, shape).astype(np.float32), rng.uniform(-0.2, 1.2, shape).astype(np.float32)      # values outside [0, 1]
    ref.flat[:4] = [0.5, np.float32(126.5 / 255), np.float32(2.5 / 255), 37 / 255.0]
    t = ref.astype(np.float32) * np.float32(255)
    ties = (t - np.floor(t)) == 0.5
    assert ties.any() and (np_grey8(ref)[ties] % 2 == 0).all() and np_grey8(ref).flat[0] == 128      # x.5 grey levels go to even
    assert np_grey8(cand).min() == 0 and np_grey8(cand).max() == 255
    assert torch.equal(Q.grey8(torch.from_numpy(ref)), torch.from_numpy(np_grey8(ref)))
    qa, qb = np_grey8(cand), np_grey8(ref)
    want = ref_quality(qa, qb, L=255.0)
    d = min(abs(ref_quality_tiled(qa, qb, L=255.0) - want[2]), abs(ref_quality(qa, qb, L=255.0, dtype=np.float32, pivot="half")[2] - want[2]))
    got = Q.restoration_quality(torch.from_numpy(ref), [torch.from_numpy(cand), torch.from_numpy(cand).half()], quantize8=True).tolist()
    print("quantize8: ssim err %.3g (tolerance %.3g), psnr err %.3g dB" % (abs(got[2] - want[2]), max(8 * d, 2.0 ** -20), abs(got[1] - want[1])))
    assert abs(got[2] - want[2]) <= max(8 * d, 2.0 ** -20) <= SSIM_CAP and abs(got[1] - want[1]) <= PSNR_TOL
    assert abs(got[0] - want[0]) <= 1e-5 * want[0]
    x = torch.from_numpy(ref)
    nan = x.clone()
    nan[0, 3, 3] = float("nan")
    assert math.isnan(Q.grey8(nan)[0, 3, 3]) and all(math.isnan(v) for v in Q.restoration_quality(x, nan, quantize8=True).tolist())
    with pytest.raises(ValueError, match="data_range must be 1"):
        Q.restoration_quality(x, x, quantize8=True, data_range=255.0)


def five_images():
    """two ordinary pairs, one identical, one with a NaN, one more ordinary; mixed sizes"""
    out = []
    for i, shape in enumerate([(3, 37, 53), (3, 70, 90), (3, 11, 75), (3, 37, 53), (1, 11, 11)]):
        a, ref = tensors(case("noise" if i % 2 else "smooth", shape, "float16", "float32"))
        if i == 2:
            a = ref.clone()
        if i == 3:
            a[1, 17, 30] = float("nan")
        out.append((ref, a))
    return out


def test_accumulator_semantics_over_five_images():
    from detectinblur_amd import quality as Q
    meter = Q.RestorationMeter("cpu", names=("blurred",))
    rows = [meter.update(ref, a).clone() for ref, a in five_images()]
    assert rows[2].tolist() == [0.0, float("inf"), 1.0] and all(math.isnan(v) for v in rows[3].tolist())
    keep = [rows[i] for i in (0, 1, 4)]
    acc = meter.acc.tolist()
    assert acc[:3] == [4.0, 1.0, 1.0]
    # the sums are the host's float64 sums of the fp32 rows, exactly and in order
    assert acc[3] == float(rows[0][0]) + float(rows[1][0]) + 0.0 + float(rows[4][0])
    assert acc[4] == float(rows[0][1]) + float(rows[1][1]) + float(rows[4][1])
    assert acc[5] == float(rows[0][2]) + float(rows[1][2]) + 1.0 + float(rows[4][2])
    meter.skip()
    res = meter.result()
    b = res["blurred"]
    assert (b["images"], b["identical"], b["nonfinite"], res["skipped"]) == (4, 1, 1, 1) and "psnr_gain_db" not in res
    assert math.isfinite(b["psnr_db"]) and b["psnr_db"] == sum(float(r[1]) for r in keep) / 3 and b["ssim"] == acc[5] / 4
    assert b["psnr_of_mean_mse_db"] == 10.0 * math.log10(1.0 / (acc[3] / 4))
    assert "blurred PSNR" in Q.format_restoration(res)
    meter.reset()
    assert meter.acc.tolist() == [0.0] * 6 and meter.skipped == 0 and meter.result()["blurred"]["images"] == 0
    two = Q.RestorationMeter("cpu")
    ref, a = five_images()[0]
    two.update(ref, a, ref)
    res = two.result()
    assert res["restored"]["identical"] == 1 and res["blurred"]["images"] == 1 and "ssim_gain" in res
    with pytest.raises(ValueError, match="sharp image"):
        two.update(ref, a[:, :20].contiguous())


def test_python_argument_checks():
    from detectinblur_amd import quality as Q
    x = torch.rand(3, 20, 30)
    with pytest.raises(ValueError, match="1 or 2 are supported"):
        Q.restoration_quality(x, [])
    with pytest.raises(ValueError, match="1 or 2 are supported"):
        Q.restoration_quality(x, [x, x, x])
    with pytest.raises(ValueError, match="shapes differ"):
        Q.restoration_quality(x, [x, x[:, :19].contiguous()])
    with pytest.raises(ValueError, match="contiguous"):
        Q.restoration_quality(x[:, :, ::2], [x[:, :, ::2]])
    with pytest.raises(ValueError, match="smaller than the 11 x 11"):
        Q.restoration_quality(x[:, :10].contiguous(), [x[:, :10].contiguous()])
    with pytest.raises(TypeError):
        Q.restoration_quality(x, [x.double()])
    with pytest.raises(ValueError, match="out must be"):
        Q.restoration_quality(x, [x, x], out=torch.zeros(3))
    with pytest.raises(ValueError, match="acc must be"):
        Q.restoration_quality(x, [x, x], acc=torch.zeros(6, dtype=torch.float64))


def test_entry_point_argument_errors_are_reported_without_a_gpu():
    """every refusal launches nothing and touches no image pointer: the addresses below are never dereferenced"""
    from detectinblur_amd import _lib
    l = _lib.lib()
    header = open(__file__.replace("tests/test_restoration_metrics.py", "include/dib.h")).read()
    assert re.search(r"\bint dib_restoration_quality\(", header) and "#define DIB_RQ_ACC_DOUBLES 6" in header
    REF, A, B, OUT, ACC, WORK = (k << 20 for k in range(1, 7))
    n = 3 * 70 * 90

    def call(ref=REF, rdt=_lib.DIB_F16, cands=(A, B), cdt=(_lib.DIB_F16, _lib.DIB_F32), K=None, C=3, H=70, W=90, q8=0, L=1.0, out=OUT,
             acc=ACC, work=WORK):
        return l.dib_restoration_quality(ref, rdt, _lib.ptr_array(list(cands)), _lib.int_array(list(cdt)), len(cands) if K is None else K,
                                         C, H, W, q8, L, out, acc, work, None)
    E, S = _lib.DIB_EINVAL, _lib.DIB_ESHAPE
    assert l.dib_restoration_quality_workspace_bytes(2, 3, 70, 90) == 2 * l.dib_image_quality_workspace_bytes(3, 70, 90) > 0
    assert l.dib_restoration_quality_workspace_bytes(3, 3, 70, 90) == 0 and l.dib_restoration_quality_workspace_bytes(1, 3, 10, 90) == 0
    for K in (0, 3):
        assert call(K=K) == E and b"1 or 2 are supported" in l.dib_last_error(), K
    for kw in (dict(ref=None), dict(out=None), dict(work=None), dict(cands=(A, None))):
        assert call(**kw) == E and b"null pointer" in l.dib_last_error(), kw
    for kw in (dict(rdt=2), dict(cdt=(0, -1))):
        assert call(**kw) == E and b"dtype" in l.dib_last_error(), kw
    for kw in (dict(H=10), dict(W=10)):
        assert call(**kw) == S and b"smaller than the 11 x 11 window" in l.dib_last_error(), kw
    assert call(C=1 << 15, H=1 << 8, W=1 << 8) == S and b"too large" in l.dib_last_error()
    assert call(q8=1, L=2.0) == E and b"data_range must be 1" in l.dib_last_error()
    assert call(L=0.0) == E and b"data_range" in l.dib_last_error()
    for kw in (dict(ref=REF + 1), dict(cands=(A, B + 2)), dict(out=OUT + 2), dict(acc=ACC + 4), dict(work=WORK + 4)):
        assert call(**kw) == E and b"misaligned" in l.dib_last_error(), kw
    for kw in (dict(out=REF + 4), dict(out=A + 2 * n - 4), dict(out=B + 4 * n - 4), dict(acc=B + 8), dict(work=A - 8), dict(out=WORK + 8),
               dict(acc=OUT + 8), dict(acc=WORK)):
        assert call(**kw) == E and b"overlap" in l.dib_last_error(), kw


_ARGV = ["--synthetic", "--synthetic_images", "2", "--synthetic_size", "128", "160", "--min_size", "128", "--max_size", "160", "--device", "cpu",
         "--blur_eval", "--tensorboard_path", ""]


@pytest.mark.parametrize("extra,message", [
    (["--gpu_blur", "--restoration_8bit"], "--restoration_8bit needs --restoration_metrics"),
    (["--gpu_blur", "--restoration_metrics", "--vanilla_eval"], "--restoration_metrics with --vanilla_eval"),
    (["--restoration_metrics", "--cpu_blur"], "--restoration_metrics needs --gpu_blur"),
    (["--restoration_metrics", "--gpu_blur", "--cpu_blur"], "--restoration_metrics needs --gpu_blur"),
    (["--restoration_metrics"], "--restoration_metrics needs --gpu_blur"),
], ids=["8bit_alone", "vanilla", "cpu_blur", "both_blurs", "no_gpu_blur"])
def test_refusals_at_start(extra, message, monkeypatch):
    from detectinblur_amd import evaluate
    monkeypatch.setattr(evaluate, "fasterrcnn_resnet50_fpn", lambda *a, **k: pytest.fail("a detector was built"))
    with pytest.raises(SystemExit, match=re.escape(message)):
        evaluate.main(evaluate.build_parser().parse_args(_ARGV + extra))


def test_engine_records_the_cell_on_the_cpu(monkeypatch):
    """3 synthetic images (one not blurred), one blurring cell, Richardson-Lucy with 2 iterations.  A "sharp" copy taken after the
    in-place blur would make every blurred image identical to it."""
    from detectinblur_amd import engine, quality as Q
    from detectinblur_amd.models import blur_functions as BF, deconvolve as DC
    from tests.test_deconvolve_first import blurring_loader, host_blur, quiet
    from tests.test_overlay import FixedDetector, fixed_detections
    monkeypatch.setattr(BF, "blur_image_list", host_blur)
    h, w, n = 40, 56, 3
    loader = blurring_loader(h, w, n, unblurred=(1,))
    cpu = torch.device("cpu")

    def run(**kw):
        model = FixedDetector(fixed_detections(h, w))
        return quiet(engine.evaluate, model, type(loader)(copy.deepcopy(list(loader))), cpu, blurring_images=True, gpu_blur=True,
                     deconvolve_first=True, deconvolver=DC.Deconvolver(iterations=2), **kw), model.seen
    plain, seen_plain = run()
    assert "restoration" not in plain and "restoration" not in plain.keys()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        model = FixedDetector(fixed_detections(h, w))
        res = engine.evaluate(model, type(loader)(copy.deepcopy(list(loader))), cpu, blurring_images=True, gpu_blur=True,
                              deconvolve_first=True, deconvolver=DC.Deconvolver(iterations=2), restoration_metrics=True)
    assert "Restoration: blurred PSNR" in buf.getvalue()
    assert all(torch.equal(a, b) for a, b in zip(model.seen, seen_plain))                   # the detector gets what it got without the flag
    r = res["restoration"]
    assert r is res.restoration and r["blurred"]["images"] + r["skipped"] == 3 and r["skipped"] == 1
    assert r["blurred"]["identical"] == 0 and math.isfinite(r["blurred"]["psnr_db"]) and r["restored"]["images"] == 2
    # an independent blur of the same images with the same blur_dicts
    rows = []
    for i in (0, 2):
        images, _, dicts = loader[i]
        sharp = images[0].half()
        mine = [sharp.clone()]
        host_blur(mine, dicts, [torch.HalfTensor(dicts[0]["psf"])])
        rows.append(Q.psnr_ssim_torch(mine[0], sharp))
    assert r["blurred"]["ssim"] == (float(rows[0][2]) + float(rows[1][2])) / 2
    assert r["blurred"]["psnr_db"] == (float(rows[0][1]) + float(rows[1][1])) / 2
    only = quiet(engine.evaluate, FixedDetector(fixed_detections(h, w)), type(loader)(copy.deepcopy(list(loader))), cpu, blurring_images=True,
                 gpu_blur=True, restoration_metrics=True, restoration_quantize8=True)["restoration"]
    assert "restored" not in only and only["quantize8"] and only["blurred"]["images"] == 2


def test_engine_scores_a_deblurrers_output_and_refuses_a_stage_that_works_in_place(monkeypatch):
    """the same cell with `deblur_first`: a stage that hands back a new tensor is scored under "restored"; one that hands back the
    tensor it was given -- the blurred image would be gone, and its pixels would be scored under the wrong name -- raises"""
    from detectinblur_amd import engine, quality as Q
    from detectinblur_amd.models import blur_functions as BF
    from tests.test_deconvolve_first import blurring_loader, host_blur, quiet
    from tests.test_overlay import FixedDetector, fixed_detections
    monkeypatch.setattr(BF, "blur_image_list", host_blur)
    h, w, n = 40, 56, 3
    loader = blurring_loader(h, w, n)
    cpu = torch.device("cpu")

    class Brighten(object):
        def __init__(self):
            self.inputs = []

        def deblur_(self, image):
            self.inputs.append(image.clone())
            return (image.float() * 0.5 + 0.25)

    class InPlace(object):
        def deblur_(self, image):
            return image.mul_(0.5)

    class Hand(object):
        def deconvolve_(self, image, blur_dict, psf, tables=None, index=0):
            return image

    def run(**kw):
        return quiet(engine.evaluate, FixedDetector(fixed_detections(h, w)), type(loader)(copy.deepcopy(list(loader))), cpu,
                     blurring_images=True, gpu_blur=True, restoration_metrics=True, **kw)["restoration"]
    stage = Brighten()
    r = run(deblur_first=True, deblurer=stage)
    assert r["restored"]["images"] == r["blurred"]["images"] == 3 and r["skipped"] == 0
    rows = []
    for i in range(n):
        sharp = loader[i][0][0].half()
        rows.append(Q.restoration_quality(sharp, [stage.inputs[i], stage.inputs[i].float() * 0.5 + 0.25]))
    assert r["blurred"]["ssim"] == sum(float(x[2]) for x in rows) / 3 and r["restored"]["ssim"] == sum(float(x[5]) for x in rows) / 3
    with pytest.raises(RuntimeError, match="handed back the tensor it was given"):
        run(deblur_first=True, deblurer=InPlace())
    with pytest.raises(RuntimeError, match="handed back the tensor it was given"):
        run(deconvolve_first=True, deconvolver=Hand())


_RANK_WORKER = r'''
import json, os, sys
sys.path.insert(0, %(root)r)
import torch
import torch.distributed as dist
from detectinblur_amd import quality as Q
dist.init_process_group("gloo")
rank = dist.get_rank()
meter = Q.RestorationMeter("cpu")
g = torch.Generator().manual_seed(3)
x = torch.rand(3, 20, 30, generator=g)
if rank == 0:                      # rank 1's shard is empty: it still takes part in the collective
    meter.update(x, (0.9 * x).half(), x)
    meter.update(x, (0.8 * x).half(), (0.95 * x))
    meter.skip()
res = meter.result()
with open(os.path.join(sys.argv[1], "rank%%d.json" %% rank), "w") as f:
    json.dump(res, f)
dist.destroy_process_group()
'''


def test_two_gloo_ranks_one_with_an_empty_shard(tmp_path):
    import json
    import os
    import subprocess
    import sys
    from tests.test_drivers_two_ranks import ROOT, _port
    worker = tmp_path / "worker.py"
    worker.write_text(_RANK_WORKER % {"root": ROOT})
    env = dict(os.environ, OMP_NUM_THREADS="2", MASTER_ADDR="127.0.0.1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_port()), str(worker), str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    a, b = (json.load(open(tmp_path / ("rank%d.json" % k))) for k in (0, 1))
    assert a == b and a["blurred"]["images"] == 2 and a["restored"]["images"] == 2 and a["restored"]["identical"] == 1 and a["skipped"] == 1
