"""The post-blur corruption chain's two HIP kernels (reference models/blur_functions.py:72-87) against
float64 restatements of the same operations (oracle/dib_oracle.py A16), element by element:

  * csrc/dib_postops.hip -- Philox-4x32-10 + Box-Muller noise, the fp16 steps of torch's Half expression, clamp, and
    the composed nearest-neighbour block maps -- against `post_ops64`: fp16 bit for bit outside the elements whose fp16
    rounding of the normal float64 cannot decide, fp32 within eps_n * std plus the two fp32 roundings;
  * csrc/dib_jpeg.hip (and the module path) against `jpeg_roundtrip64`: every pixel within its stated bound, one fp16
    rounding plus the fp32 chain's error away from any coefficient that may round either way.

The CPU half pins the references themselves: Random123's known answers, the reference's own JPEG goldens, the module
path of this package, and the block goldens; plus the drop-in's CPU chain against the reference (tests/golden/
postops_chain.npz) and the 2-D image + block draw, which must raise as the reference does."""
import math
import os

import numpy as np
import pytest
import torch

import dib_oracle as O
import gen_goldens as GG
from detectinblur_amd import transforms as T
from detectinblur_amd.models import blur_functions as BF
from detectinblur_amd.models.jpeg import DiffJPEG, quality_to_factor

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# eps_n: bound on |normal of the kernel (__logf, __cosf, sqrtf, fp32 products) - normal64|.  A MEASUREMENT, not a
# derivation: on an MI355X, test_noise_normal_error_is_within_eps_n found max |n_gpu - n64| = 2.006e-6 over 3 x 600 x 600
# elements (n recovered as (out - 0.5) / 0.05 from an fp32 image of 0.5, which adds up to ~1.2e-6 of the recovery's own
# fp32 rounding); eps_n is that figure with a margin of 2x.
EPS_N = 4e-6


def _image(shape, rs, kind="mixed", dtype=np.float32):
    """3 x H x W test images: smooth + texture, flat blocks, saturated primaries, white noise."""
    C, H, W = shape
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    if kind == "noise":
        img = rs.uniform(0, 1, shape)
    elif kind == "flat":
        img = np.stack([np.full((H, W), v) for v in rs.uniform(0, 1, C)])
        img[:, H // 3:, W // 2:] = rs.uniform(0, 1, (C, 1, 1))          # two flat regions, one edge
    elif kind == "primaries":
        img = (rs.uniform(0, 1, shape) > 0.5).astype(np.float64)        # every pixel 0 / 1 per channel
        img[:, ::7] = np.array([1.0, 0.0, 0.0])[:C, None, None]         # pure red rows: the RGB clamp engages
    else:
        img = np.stack([0.5 + 0.4 * np.sin(6 * xx + c) * np.cos(4 * yy) for c in range(C)]) + rs.uniform(-0.08, 0.08, shape)
    return np.clip(img, 0, 1).astype(dtype)


def _tables(q):
    f = np.float32(quality_to_factor(q))
    return O.JPEG_LUMA * f, O.JPEG_CHROMA * f


def _check_jpeg(got, img, q, what):
    exp, bound, exact = O.jpeg_roundtrip64(img, q)
    d = np.abs(np.asarray(got, dtype=np.float64) - exp)
    bad = d > bound
    assert got.shape == exp.shape and not bad.any(), (
        "%s q=%g: %d pixels outside their bound (worst |d| / bound %.3g at %s); unambiguous fraction %.3f"
        % (what, q, int(bad.sum()), float((d / bound).max()), np.unravel_index(int(np.argmax(d / bound)), d.shape), exact.mean()))
    return exact.mean()


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_philox4x32_10_known_answers():
    """Random123's three Philox4x32-10 known-answer vectors (kat_vectors)."""
    cases = (([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
             ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
             ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
              [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]))
    for ctr, key, want in cases:
        assert O.philox4x32_10(np.array(ctr, dtype=np.uint32), key).tolist() == want
    both = O.philox4x32_10(np.array([c for c, _, _ in cases[:1]] * 3, dtype=np.uint32), cases[0][1])
    assert (both == np.array(cases[0][2], dtype=np.uint32)).all()           # vectorised over counters


def test_oracle_tables_are_the_modules():
    m = DiffJPEG(height=100, width=100, differentiable=False, quality=10)
    assert np.array_equal(m.luma.numpy(), O.JPEG_LUMA) and np.array_equal(m.chroma.numpy(), O.JPEG_CHROMA)
    for q in (10, 20, 49, 49.9, 50, 51, 75, 90, 95):
        assert O.jpeg_quality_factor(q) == quality_to_factor(q)


@pytest.mark.parametrize("q", GG.JPEG_QUALITIES)
def test_jpeg64_reproduces_the_references_goldens(golden, q):
    """tests/golden/jpeg.npz: the reference's DiffJPEG on 32 x 48 (no padding) -- every pixel within its bound, and
    most pixels in blocks without an ambiguous coefficient (so the mask cannot swallow a case)."""
    x = GG.jpeg_input().numpy()
    for i in range(x.shape[0]):
        exp, bound, exact = O.jpeg_roundtrip64(x[i], q, pad=False)
        d = np.abs(golden.jpeg["jpeg_q%d" % q][i].astype(np.float64) - exp)
        assert (d <= bound).all(), (q, i, float((d / bound).max()))
        assert d[:, exact].max() <= 1e-6, (q, i)          # fp32 output: far inside the fp16 part of the bound
        assert exact.mean() >= 0.4, (q, i, exact.mean())


@pytest.mark.parametrize("shape", [(3, 37, 50), (3, 64, 64), (3, 17, 200), (3, 203, 160), (3, 18, 18)])
def test_jpeg64_equals_the_module_path_on_cpu(shape):
    """transforms.add_jpeg_artifact_to_image on the CPU (reflect pad, DiffJPEG module, crop, .half()) at padded and edge
    sizes -- 64 x 64 gets a full extra macroblock -- and qualities on both sides of quality_to_factor's q < 50 branch."""
    m = DiffJPEG(height=100, width=100, differentiable=False, quality=10)
    rs = np.random.RandomState(shape[1] * 1000 + shape[2])
    for k, q in enumerate((20, 49, 50, 51, 75, 90, 95)):
        img = _image(shape, rs, ("mixed", "noise", "flat", "primaries")[k % 4], (np.float32, np.float16)[k % 2])
        got = T.add_jpeg_artifact_to_image(torch.from_numpy(img), m, q)
        assert got.dtype == torch.float16
        frac = _check_jpeg(got.numpy(), img, q, "cpu module %s" % (shape,))
        assert frac >= 0.25 or k % 4 == 1, (shape, q, frac)        # white noise: most blocks have some ambiguity


def test_post_ops64_block_arm_equals_the_references_goldens():
    """tests/golden/postops.npz block cases (the reference on the CPU): the composed index maps of post_ops64 bit for
    bit, after the reference's own coin flip and scale draw."""
    G = np.load(os.path.join(GOLDEN, "postops.npz"))
    x, _ = GG.postop_input()
    x = x.numpy()
    landed = []
    for seed in GG.POSTOP_SEEDS:
        np.random.seed(seed)
        s = np.random.uniform(0.6, 1) if np.random.uniform(0, 1) > 0.5 else None
        got, undet = O.post_ops64(x, None, s, seed, EPS_N)
        assert not undet.any() and np.array_equal(got, G["block_%d" % seed]), seed
        landed.append(s is not None)
    assert any(landed) and not all(landed)


def test_post_ops64_fp16_noise_follows_the_kernels_rounding_steps():
    """The fp16 arm: out = half(v + half(half(n) * std)), clamped; the not-determined set (n within eps_n of an fp16
    rounding boundary, and the two candidate halves giving different outputs) is small."""
    rs = np.random.RandomState(2)
    x = rs.uniform(0, 1, (3, 30, 70)).astype(np.float16)
    out, undet = O.post_ops64(x, 0.01, None, 7, EPS_N)
    assert out.dtype == np.float16 and out.shape == x.shape and undet.mean() < 0.05
    n = O.normal64(np.arange(x.size, dtype=np.uint64), O.post_ops_key(7)).reshape(x.shape)
    assert abs(n.mean()) < 0.05 and abs(n.std() - 1) < 0.03
    prod = (n.astype(np.float16).astype(np.float32) * np.float32(0.1)).astype(np.float16)
    want = np.clip((x.astype(np.float32) + prod.astype(np.float32)).astype(np.float16), 0, 1)
    assert np.array_equal(out, want)


def test_cpu_chain_equals_the_reference_with_jpeg():
    """tests/golden/postops_chain.npz: the reference's manual_blur (noise, block, JPEG via
    add_jpeg_artifact_to_image + DiffJPEG) on the CPU; the drop-in's CPU path equals it bit for bit, dtype included, and
    leaves numpy's global stream where the reference left it.  The seeds cover both arms of the JPEG coin."""
    G = np.load(os.path.join(GOLDEN, "postops_chain.npz"))
    x, _ = GG.postop_input()
    m = DiffJPEG(height=100, width=100, differentiable=False, quality=10)
    dtypes = set()
    for seed in GG.POSTOP_CHAIN_SEEDS:
        np.random.seed(seed); torch.manual_seed(seed)
        with torch.no_grad():
            got = BF._post_ops(x.clone(), True, 0.004, True, True, m).numpy()
        want = G["chain_%d" % seed]
        assert got.dtype == want.dtype and np.array_equal(got, want), seed
        assert np.random.uniform() == G["chain_rng_after_%d" % seed][0], seed
        dtypes.add(want.dtype.name)
    assert dtypes == {"float16", "float32"}                 # both arms of the > 0.35 coin


def _draws_2d(seed, add_block):
    """The reference's draws on numpy's stream for noise (+ block): (block coin landed, the next uniform)."""
    np.random.seed(seed)
    np.random.uniform(0.00000001, 0.001)
    landed = False
    if add_block and np.random.uniform(0, 1) > 0.5:
        np.random.uniform(0.6, 1)
        landed = True
    return landed, np.random.uniform()


def _run_2d(img, seed, add_block):
    np.random.seed(seed); torch.manual_seed(seed)
    try:
        out, err = BF._post_ops(img.clone(), True, 0.001, add_block, False, None), None
    except Exception as e:          # noqa: BLE001 -- the type is what is compared
        out, err = None, type(e)
    return out, err, np.random.uniform()


def _expected_2d_error():
    try:
        torch.nn.functional.interpolate(torch.zeros(1, 5, 6), scale_factor=(0.7, 0.7), mode="nearest")
    except Exception as e:          # noqa: BLE001
        return type(e)
    raise AssertionError("interpolate accepted a 3-D input with two scale factors")


def test_2d_image_with_a_block_draw_raises_like_the_reference_on_cpu():
    """A one-channel image reaches _post_ops as H x W (manual_blur squeezes it); the reference's block arm then calls
    interpolate on a 3-D tensor with two scale factors and raises.  Noise alone passes; numpy's stream is consumed the
    same way in every case."""
    err_type = _expected_2d_error()
    img = torch.rand(40, 56, generator=torch.Generator().manual_seed(3))
    seen = set()
    for seed in range(6):
        landed, after = _draws_2d(seed, True)
        out, err, got_after = _run_2d(img, seed, True)
        assert got_after == after and (err is err_type if landed else err is None and out.shape == img.shape), seed
        seen.add(landed)
        _, after = _draws_2d(seed, False)
        out, err, got_after = _run_2d(img, seed, False)
        assert err is None and out.shape == img.shape and got_after == after
    assert seen == {True, False}


# ---------------------------------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
def test_2d_image_with_a_block_draw_raises_like_the_reference_on_gpu():
    err_type = _expected_2d_error()
    for dt in (torch.float16, torch.float32):
        img = torch.rand(40, 56, generator=torch.Generator().manual_seed(3)).to(dt).cuda()
        seen = set()
        for seed in range(6):
            landed, after = _draws_2d(seed, True)
            out, err, got_after = _run_2d(img, seed, True)
            assert got_after == after and (err is err_type if landed else err is None and out.shape == img.shape), (dt, seed)
            seen.add(landed)
            _, after = _draws_2d(seed, False)
            out, err, got_after = _run_2d(img, seed, False)
            assert err is None and out.shape == img.shape and out.is_cuda and got_after == after
        assert seen == {True, False}


@pytest.mark.gpu
def test_noise_normal_error_is_within_eps_n():
    """The one measured number: the kernel's normal against normal64 over 3 x 600 x 600 elements, recovered from an fp32
    image of 0.5 with std 0.05 (nothing clamps: |n| < 10)."""
    from detectinblur_amd import blur_ops
    x = torch.full((3, 600, 600), 0.5, device="cuda")
    torch.manual_seed(123)
    out = blur_ops.post_ops(x, 0.05 ** 2, None).cpu().numpy().astype(np.float64)
    n_gpu = (out - 0.5) / np.float64(np.float32(0.05))
    n64 = O.normal64(np.arange(x.numel(), dtype=np.uint64), O.post_ops_key(123)).reshape(out.shape)
    err = float(np.abs(n_gpu - n64).max())
    print("eps_n measured: max |n_gpu - n64| = %.4g over %d elements" % (err, x.numel()))
    assert err <= EPS_N, err


def _noise_cases():
    # (shape, dtype, noise_var, block_scale): 800 x 1333 is the size the chain sees; the other widths leave a ragged last
    # 256-column tile of the grid; both ends of the reference's variance draw uniform(1e-8, noise_level <= 0.01)
    return [((3, 800, 1333), np.float16, 0.01, None), ((3, 800, 1333), np.float32, 0.01, 0.8123),
            ((3, 97, 517), np.float16, 1e-8, 0.7), ((1, 123, 300), np.float16, 0.01, None),
            ((1, 64, 257), np.float32, 1e-8, None), ((3, 61, 770), np.float32, 0.004, None),
            ((3, 45, 259), np.float16, 0.004, 0.6), ((1, 200, 511), np.float16, 0.01, 0.93)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(8))
def test_fused_noise_equals_post_ops64(case):
    from detectinblur_amd import blur_ops
    shape, dt, var, s = _noise_cases()[case]
    rs = np.random.RandomState(case)
    x = rs.uniform(0, 1, shape)
    x[:, ::9] = np.round(x[:, ::9])                      # 0 / 1 rows: the clamp at both ends
    x = x.astype(dt)
    img = torch.from_numpy(x).cuda()
    if shape[0] == 1 and case % 2:
        img, x = img[0], x[0]                            # H x W, as manual_blur hands a squeezed one-channel image on
    seed = 1000 + case
    torch.manual_seed(seed)
    got = blur_ops.post_ops(img, var, s).cpu().numpy()
    want, undet = O.post_ops64(x, var, s, seed, EPS_N)
    assert got.dtype == want.dtype and got.shape == want.shape
    if dt == np.float16:
        diff = got.view(np.uint16) != want.view(np.uint16)
        assert not (diff & ~undet).any(), (case, int((diff & ~undet).sum()), np.argwhere(diff & ~undet)[:5].tolist())
        assert undet.mean() <= 0.05, (case, undet.mean())
    else:
        std = float(np.float32(math.sqrt(var)))
        n = O.normal64(np.arange(x.size, dtype=np.uint64), O.post_ops_key(seed)).reshape(x.shape)
        sy, sx = O.block_source_map(x.shape[-2], x.shape[-1], s)
        n = (n[None] if n.ndim == 2 else n)[:, sy][:, :, sx].reshape(want.shape)
        ulp = lambda a: np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)        # noqa: E731
        tol = EPS_N * std + ulp(want) + 2 * ulp(n * std)     # the normal's error, the sum's and the product's roundings
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        assert (d <= tol).all(), (case, float((d / tol).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(6))
def test_fused_jpeg_kernel_equals_jpeg64(case):
    """csrc/dib_jpeg.hip, through blur_ops.jpeg_roundtrip and through add_jpeg_artifact_to_image, every pixel within
    jpeg_roundtrip64's bound: 800 x 1333 (H % 16 == 0: a full extra macroblock row; 1333: an 11-column pad), ragged and
    tiny sizes, fp16 / fp32 and non-contiguous inputs, saturated primaries, flat blocks and white noise, q 20..95."""
    from detectinblur_amd import blur_ops
    shape, kinds, qs = [((3, 800, 1333), ("mixed", "primaries"), (20, 50)), ((3, 37, 50), ("noise", "flat"), (49, 51, 95)),
                        ((3, 17, 200), ("mixed", "primaries"), (25, 90)), ((3, 16, 16), ("flat", "noise"), (50, 75)),
                        ((3, 18, 18), ("primaries", "mixed"), (20, 49, 95)), ((3, 203, 160), ("noise", "flat"), (33, 51))][case]
    m = DiffJPEG(height=100, width=100, differentiable=False, quality=10).cuda()
    rs = np.random.RandomState(40 + case)
    fracs = []
    for k, q in enumerate(qs):
        dt = (np.float16, np.float32)[(k + case) % 2]
        img = _image(shape, rs, kinds[k % 2], dt)
        if k == 1:          # non-contiguous: a channels-last buffer seen as C x H x W
            g = torch.from_numpy(np.ascontiguousarray(img.transpose(1, 2, 0))).cuda().permute(2, 0, 1)
            assert not g.is_contiguous()
        else:
            g = torch.from_numpy(img).cuda()
        qy, qc = _tables(q)
        fracs.append(_check_jpeg(blur_ops.jpeg_roundtrip(g, qy, qc).cpu().numpy(), img, q, "blur_ops %s %s" % (shape, dt.__name__)))
        got = T.add_jpeg_artifact_to_image(g, m, q)
        assert got.device.type == "cpu" and got.dtype == torch.float16
        _check_jpeg(got.numpy(), img, q, "add_jpeg_artifact_to_image %s" % (shape,))
    print("unambiguous fractions", shape, dict(zip(qs, np.round(fracs, 3))))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 37, 50), (3, 64, 64), (3, 203, 160)])
def test_module_path_on_gpu_equals_jpeg64(shape):
    """The module path on the GPU (FUSE_JPEG off: the tensordots as GEMMs) -- the bound's delta already covers a 64-term
    sum in any order, so the same reference and bound hold."""
    m = DiffJPEG(height=100, width=100, differentiable=False, quality=10).cuda()
    rs = np.random.RandomState(shape[2])
    try:
        T.FUSE_JPEG = False
        for k, q in enumerate((20, 49, 51, 90)):
            img = _image(shape, rs, ("mixed", "primaries", "noise", "flat")[k], (np.float16, np.float32)[k % 2])
            _check_jpeg(T.add_jpeg_artifact_to_image(torch.from_numpy(img).cuda(), m, q).numpy(), img, q, "module gpu %s" % (shape,))
    finally:
        T.FUSE_JPEG = True
