"""AugMix on the host (transforms.AugMix, augmix.draw_plan / apply_plan) against the reference's T.AugMix (transforms.py:68-79 around
augmix/augment_and_mix.py), the drivers' flags, and the device kernels' resources.

  * Hundreds of seeds at small odd sizes, a few at 800 x 1333, with and without positional ops and box expansion: image and boxes
    equal bit for bit, and Python's `random` and numpy's global stream end in the same state.
  * The deferred plan (pixels left to the GPU) applied on the host equals the immediate path, with and without a later flip.
  * tests/golden/augmix.npz pins the same against recorded reference outputs where the reference tree is absent
    (`python tests/test_augmix.py --write` regenerates it from the live reference).
  * `train.main --synthetic --non_pos_aug_mix --include_pos_aug_mix --aug_mix_target_expand` runs a CPU step.
  * hipcc's resource report of csrc/dib_augmix.hip shows no scratch.
"""
import copy
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from detectinblur_amd import augmix as A  # noqa: E402
from detectinblur_amd import transforms as T  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "augmix.npz")
SIZES = [(7, 5), (13, 17), (31, 23), (9, 40)]


def _foreign(mod, root):
    """A module ref_harness.load() put into sys.modules that must not outlive the comparison: one of its stubs (MagicMocks, the cv2
    shim) or a module of the reference tree (whose generic top-level names -- utils, transforms, models -- shadow others)."""
    from unittest import mock
    if isinstance(mod, mock.MagicMock) or getattr(mod, "__name__", None) == "cv2":
        return True
    places = [getattr(mod, "__file__", None) or ""] + list(getattr(mod, "__path__", None) or [])
    return any(str(p).startswith(root) for p in places)


class _Isolated(object):
    """The reference for a block of comparisons, without leaking into later test files: ref_harness.load() installs stub modules
    (torchvision, torch.utils.tensorboard, cv2, ...), the reference's top-level modules and its directory on sys.path.  The
    namespace it returns keeps its own references; sys.modules, sys.path, numpy's `math` alias and the harness's cache are put back
    right after loading, so a later load() starts afresh."""

    def __enter__(self):
        modules, path, np_math = dict(sys.modules), list(sys.path), hasattr(np, "math")
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        try:
            import ref_harness
            if not ref_harness.available():
                pytest.skip("reference tree not present")
            loaded = dict(ref_harness._loaded)
            try:
                return ref_harness.load()
            finally:
                root = os.path.realpath(ref_harness.REFERENCE_ROOT)
                for name in [k for k in sys.modules if k not in modules or sys.modules[k] is not modules[k]]:
                    if _foreign(sys.modules[name], root):
                        del sys.modules[name]
                sys.modules.update({k: v for k, v in modules.items() if k not in sys.modules})
                ref_harness._loaded.clear()
                ref_harness._loaded.update(loaded)
                if not np_math and hasattr(np, "math"):
                    del np.math
        finally:
            sys.path[:] = path

    def __exit__(self, *exc):
        return False


@pytest.fixture(scope="module")
def reference():
    with _Isolated() as R:
        yield R


def _case(seed, H, W, nb=5):
    """A uint8 image (every 7th one constant: degenerate histograms) and boxes partly outside it."""
    g = np.random.RandomState(seed)
    img = np.full((H, W, 3), seed % 256, np.uint8) if seed % 7 == 0 else g.randint(0, 256, (H, W, 3)).astype(np.uint8)
    x1, y1 = g.uniform(-5, W, nb), g.uniform(-5, H, nb)
    b = np.stack([x1, y1, x1 + g.uniform(0, W / 2, nb), y1 + g.uniform(0, H / 2, nb)], 1).astype(np.float32)
    return img, {"boxes": torch.from_numpy(b), "labels": torch.arange(nb)}


def _flags(seed):
    return bool(seed & 1), bool(seed & 2)       # positional ops, box expansion


def _run(transform, img, target, seed):
    np.random.seed(seed)
    random.seed(seed)
    out, tg, bd = transform(Image.fromarray(img), copy.deepcopy(target), {})
    st = np.random.get_state()
    return np.asarray(out), tg["boxes"].numpy(), (st[1].copy(), st[2], st[3], st[4]), random.getstate(), bd


def _same_state(a, b):
    return np.array_equal(a[0], b[0]) and a[1:] == b[1:]


@pytest.mark.parametrize("block", range(4))
def test_host_path_equals_reference_small_sizes(block, reference):
    R = reference
    for seed in range(block * 100, block * 100 + 100):
        H, W = SIZES[seed % 4]
        pos, mod = _flags(seed)
        img, tg = _case(seed, H, W)
        ri, rb, rs, rr, _ = _run(R.transforms.AugMix(include_pos_aug_mix=pos, modify_target_boxes=mod), img, tg, seed)
        mi, mb, ms, mr, bd = _run(T.AugMix(include_pos_aug_mix=pos, modify_target_boxes=mod), img, tg, seed)
        assert np.array_equal(ri, mi), (seed, bd["augmix"]["chains"])
        assert np.array_equal(rb, mb), (seed, bd["augmix"]["chains"])
        assert _same_state(rs, ms) and rr == mr, seed
        if not mod:
            assert np.array_equal(mb, tg["boxes"].numpy())


def test_host_path_equals_reference_800x1333(reference):
    R = reference
    for seed in (1, 2, 3, 4):
        img, tg = _case(seed + 1000, 800, 1333, nb=8)
        pos, mod = _flags(seed)
        ri, rb, rs, rr, _ = _run(R.transforms.AugMix(include_pos_aug_mix=pos, modify_target_boxes=mod), img, tg, seed)
        mi, mb, ms, mr, _ = _run(T.AugMix(include_pos_aug_mix=pos, modify_target_boxes=mod), img, tg, seed)
        assert np.array_equal(ri, mi) and np.array_equal(rb, mb) and _same_state(rs, ms) and rr == mr, seed


def test_deferred_plan_equals_immediate_path_with_and_without_flip():
    for seed in range(60):
        H, W = SIZES[seed % 4]
        pos, mod = _flags(seed)
        img, tg = _case(seed, H, W)
        mi, mb, ms, mr, _ = _run(T.AugMix(include_pos_aug_mix=pos, modify_target_boxes=mod), img, tg, seed)
        # deferred, the synthetic dataset's float tensor in: same draws, same boxes, pixels untouched
        x = torch.from_numpy(img.transpose(2, 0, 1).astype(np.float32) / 255)
        np.random.seed(seed)
        random.seed(seed)
        flip = T.RandomHorizontalFlip(1.0 if seed % 3 else 0.0)
        t = T.Compose([T.AugMix(include_pos_aug_mix=pos, modify_target_boxes=mod, defer=True), T.ToTensor(), flip])
        out, tg2, bd = t(x, copy.deepcopy(tg), {})
        plan = bd["augmix"]
        assert plan["deferred"] and plan["flip"] == bool(seed % 3)
        assert torch.equal(out, torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1)[:, :, ::-1 if plan["flip"] else 1])).float().div(255))
        want = T.to_tensor(Image.fromarray(mi))
        if plan["flip"]:
            want = want.flip(-1)
            mb = mb.copy()
            mb[:, [0, 2]] = W - mb[:, [2, 0]]
        assert torch.equal(A.apply_deferred_host(out, plan), want), seed
        assert np.array_equal(tg2["boxes"].numpy(), mb), seed
        st = np.random.get_state()
        assert _same_state((st[1].copy(), st[2], st[3], st[4]), ms)


def test_synthetic_tensor_gives_augmix_the_pil_images_uint8():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(3, 21, 34, generator=g)
    pil = np.asarray(Image.fromarray((x.permute(1, 2, 0).numpy() * 255).astype(np.uint8)))   # coco_utils' as_tensor=False image
    assert np.array_equal(A.to_uint8_hwc(x), pil)
    np.random.seed(0)
    out, _, _ = T.AugMix(defer=True)(x, {"boxes": torch.zeros(0, 4)}, {})
    assert torch.equal(out, torch.from_numpy(pil.transpose(2, 0, 1).copy()).float().div(255))


def test_draw_order_and_parameter_ranges():
    np.random.seed(5)
    for _ in range(300):
        plan, _ = A.draw_plan(50, 70, positional=True)
        assert len(plan["chains"]) == 3 and all(1 <= len(c) <= 3 for c in plan["chains"])
        assert np.float32(plan["m"]) == plan["m"] and abs(sum(plan["ws"]) - 1) < 1e-5
        for op, p in (x for c in plan["chains"] for x in c):
            if op == A.POSTERIZE:
                assert 1 <= p <= 4
            elif op == A.SOLARIZE:
                assert 1 <= p <= 256
            elif op == A.ROTATE:
                assert -11 <= p <= 11
            elif op in (A.SHEAR_X, A.SHEAR_Y):
                assert abs(p) < 0.12
            elif op in (A.TRANSLATE_X, A.TRANSLATE_Y):
                assert abs(p) <= 8


# ---- golden fixture ----------------------------------------------------------------------------------------------------------

GOLDEN_SEEDS = list(range(24))


def build_fixture(R):
    out = {}
    for seed in GOLDEN_SEEDS:
        H, W = SIZES[seed % 4]
        pos, mod = _flags(seed)
        img, tg = _case(seed, H, W)
        ri, rb, rs, rr, _ = _run(R.transforms.AugMix(include_pos_aug_mix=pos, modify_target_boxes=mod), img, tg, seed)
        out["img_%d" % seed], out["boxes_%d" % seed], out["pos_%d" % seed] = ri, rb, rs[1]
    return out


def test_host_path_equals_recorded_reference_outputs():
    fx = np.load(GOLDEN)
    for seed in GOLDEN_SEEDS:
        H, W = SIZES[seed % 4]
        pos, mod = _flags(seed)
        img, tg = _case(seed, H, W)
        mi, mb, ms, _, _ = _run(T.AugMix(include_pos_aug_mix=pos, modify_target_boxes=mod), img, tg, seed)
        assert np.array_equal(fx["img_%d" % seed], mi), seed
        assert np.array_equal(fx["boxes_%d" % seed], mb), seed
        assert int(fx["pos_%d" % seed]) == ms[1], seed


# ---- drivers ----------------------------------------------------------------------------------------------------------------

def test_flags_are_accepted_and_reach_the_transform():
    from detectinblur_amd import evaluate as EV
    from detectinblur_amd import train as TR
    a = TR.build_parser().parse_args(["--non_pos_aug_mix", "--include_pos_aug_mix", "--aug_mix_target_expand"])
    TR.reject_out_of_scope(a)
    e = EV.build_parser().parse_args(["--non_pos_aug_mix", "--include_pos_aug_mix", "--aug_mix_target_expand"])
    TR.reject_out_of_scope(e)
    tf = TR.get_transform(True, blur=True, non_pos_aug_mix=True, include_pos_aug_mix=True, aug_mix_target_expand=True, defer_aug_mix=True)
    assert [type(t).__name__ for t in tf.transforms] == ["AugMix", "BlurImage", "ToTensor", "RandomHorizontalFlip"]
    am = tf.transforms[0]
    assert am.include_pos_aug_mix and am.modify_target_boxes and am.defer
    assert not TR.get_transform(True, cpu_blur=True, non_pos_aug_mix=True, defer_aug_mix=True).transforms[0].defer
    assert [type(t).__name__ for t in TR.get_transform(True, include_pos_aug_mix=True).transforms] == ["ToTensor", "RandomHorizontalFlip"]


def test_train_main_runs_a_cpu_step_with_augmix(tmp_path, monkeypatch):
    import detectinblur_amd.train as TR
    from detectinblur_amd import engine
    from tests.test_engine_ddp_cpu import _small_model
    monkeypatch.setattr(TR, "fasterrcnn_resnet50_fpn", lambda **kw: _small_model())
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    seen = []
    real = engine._stage

    def spy(images_CPU, targets, blur_dicts, *a):
        seen.append([bd.get("augmix") for bd in blur_dicts])
        return real(images_CPU, targets, blur_dicts, *a)
    monkeypatch.setattr(engine, "_stage", spy)
    argv = ["--synthetic", "--synthetic_images", "2", "--synthetic_size", "90", "120", "--device", "cpu", "-b", "2", "--epochs", "1",
            "--non_pos_aug_mix", "--include_pos_aug_mix", "--aug_mix_target_expand", "--output_dir", "", "--tensorboard_path", "",
            "--print_freq", "1", "--lr", "0.001"]
    TR.main(TR.build_parser().parse_args(argv))
    plans = [p for batch in seen for p in batch if p is not None]
    assert plans and not any(p["deferred"] for p in plans)      # a CPU run applies the plans in the loader


# ---- kernel resources -------------------------------------------------------------------------------------------------------

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_augmix_kernels_use_no_scratch():
    if not os.path.isfile(HIPCC):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "detectinblur_amd", "csrc", "dib_augmix.hip")
    p = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-c", src,
                        "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    out, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    for frag in ("augmix_hist_kernel", "augmix_lut_kernel", "augmix_stage_kernel", "augmix_mix_kernel"):
        names = [n for n in out if frag in n]
        assert names, frag
        for n in names:
            assert out[n]["ScratchSize"] == 0, (n, out[n])
            assert out[n]["Occupancy"] >= 4, (n, out[n])


if __name__ == "__main__":
    if "--write" in sys.argv:
        with _Isolated() as R:
            np.savez_compressed(GOLDEN, **build_fixture(R))
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
