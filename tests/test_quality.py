"""Restoration quality on the host: quality.psnr_ssim's torch restatement (what `--device cpu` runs) against a float64 numpy statement of
the definition written here; its closed forms; its behaviour on the stage it is for; the C entry point's argument checks; the deblurrer
trainer's validation line.  tests/test_quality_gpu.py holds the HIP kernel to the same float64 reference with the same tolerance rule.

The definition (include/dib.h, dib_image_quality): Wang et al. 2004 as skimage.metrics.structural_similarity(gaussian_weights=True,
sigma=1.5, use_sample_covariance=False, data_range=L, channel_axis=0) computes it.
    mse = mean (a - b)^2;  psnr_db = 10 log10(L^2 / mse), +inf when mse == 0
    g: 11 taps, g_k ~ exp(-(k - 5)^2 / (2 1.5^2)), sum 1; every moment the valid 11 x 11 correlation with g (x) g
    var_a = E[aa] - mu_a^2, var_b = E[bb] - mu_b^2, cov = E[ab] - mu_a mu_b;  C1 = (0.01 L)^2, C2 = (0.03 L)^2
    S = (2 mu_a mu_b + C1)(2 cov + C2) / ((mu_a^2 + mu_b^2 + C1)(var_a + var_b + C2));  ssim = mean S

Tolerances.  SSIM: max(8 min(d, d_half), 2^-20), the rule of tests/test_deconvolve_first.py: d = the deviation from float64 of a float32
numpy restatement of the kernel's arithmetic as include/dib.h describes it, computed here at run time from the reference alone -- per
32 x 32 tile of windows the pixels of its 42 x 42 tile (clamped at the image's edge) minus their float32 mean, moments and S in float32,
the pivot added back to the means; 2^-20 = 16 ulp of a value near 1; the factor 8 covers another summation order and fused
multiply-adds.  d_half is the same with the fixed shift by L / 2; taking the smaller of the two keeps the bound at or below what the
L / 2 form alone would give.  No case may need more than 1e-4.  (The L / 2 form by itself cannot serve as the arithmetic: on the
near-flat pair E[x x] - mu^2 cancels at ulp(0.16) = 1.5e-8 against C2 = 9e-4, and a single window is off by 2e-7 .. 1e-4 depending on
the draw: 8 d_half is above the cap for most draws at 1 x 11 x 11.)
PSNR: 1e-3 dB (fp32 partials of a handful of squares, fp64 across them: the mse is good to ~2e-6 relative, 1e-5 dB)."""
import contextlib
import functools
import io
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SSIM_CAP = 1e-4
PSNR_TOL = 1e-3


# ---- the float64 statement -----------------------------------------------------------------------------------------------------------

def ref_window(dtype=np.float64):
    k = np.arange(11, dtype=np.float64)
    g = np.exp(-(k - 5.0) ** 2 / (2.0 * 1.5 ** 2))
    return (g / g.sum()).astype(dtype)


def ref_moment(x, dtype=np.float64):
    """valid 11 x 11 correlation of every plane of x (C x H x W) with g (x) g: rows, then columns"""
    g = ref_window(dtype)
    C, H, W = x.shape
    rows = np.zeros((C, H, W - 10), dtype=dtype)
    for k in range(11):
        rows = rows + g[k] * x[:, :, k:k + W - 10]
    out = np.zeros((C, H - 10, W - 10), dtype=dtype)
    for k in range(11):
        out = out + g[k] * rows[:, k:k + H - 10, :]
    return out


def ref_quality(a, b, L=1.0, dtype=np.float64, pivot="mean"):
    """(mse, psnr_db, ssim).  float64: the definition as it stands.  float32: pixels minus a pivot ("half": L / 2; "mean": the plane's
    float32 mean, per image -- ref_quality_tiled has the kernel's per-tile pivot), moments and S in float32, the two means over the image
    in float64."""
    a, b, T = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype), dtype
    d = (a - b).astype(np.float64)
    mse = float(np.mean(d * d))
    with np.errstate(divide="ignore", invalid="ignore"):
        psnr = float(10.0 * np.log10(L * L / mse)) if mse != 0 else float("inf")
    if dtype != np.float32:
        shift_a = shift_b = T(0)
    elif pivot == "half":
        shift_a = shift_b = T(0.5 * L)
    else:
        shift_a, shift_b = a.mean(axis=(1, 2), keepdims=True, dtype=T), b.mean(axis=(1, 2), keepdims=True, dtype=T)
    x, y = a - shift_a, b - shift_b
    ma, mb = ref_moment(x, T), ref_moment(y, T)
    va, vb, cab = ref_moment(x * x, T) - ma * ma, ref_moment(y * y, T) - mb * mb, ref_moment(x * y, T) - ma * mb
    mua, mub = ma + shift_a, mb + shift_b
    c1, c2 = T((0.01 * L) ** 2), T((0.03 * L) ** 2)
    S = ((T(2) * mua * mub + c1) * (T(2) * cab + c2)) / ((mua * mua + mub * mub + c1) * (va + vb + c2))
    return mse, psnr, float(np.mean(S.astype(np.float64)))


TILE = 32          # windows per tile side: csrc/dib_quality.hip's Q_TW = Q_TH


def ref_quality_tiled(a, b, L=1.0):
    """ssim by the float32 restatement of the kernel's stated arithmetic: every TILE x TILE tile of windows on its own, its (TILE + 10)^2
    pixels (coordinates clamped into the image) shifted by their float32 mean, one pivot per image"""
    T = np.float32
    a, b = np.asarray(a).astype(T), np.asarray(b).astype(T)
    C, H, W = a.shape
    c1, c2 = T((0.01 * L) ** 2), T((0.03 * L) ** 2)
    total = 0.0
    for y0 in range(0, H - 10, TILE):
        for x0 in range(0, W - 10, TILE):
            gy, gx = np.minimum(y0 + np.arange(TILE + 10), H - 1), np.minimum(x0 + np.arange(TILE + 10), W - 1)
            ta, tb = a[:, gy][:, :, gx], b[:, gy][:, :, gx]
            pa, pb = ta.mean(axis=(1, 2), keepdims=True, dtype=T), tb.mean(axis=(1, 2), keepdims=True, dtype=T)
            x, y = ta - pa, tb - pb
            ma, mb = ref_moment(x, T), ref_moment(y, T)
            va, vb, cab = ref_moment(x * x, T) - ma * ma, ref_moment(y * y, T) - mb * mb, ref_moment(x * y, T) - ma * mb
            mua, mub = ma + pa, mb + pb
            S = ((T(2) * mua * mub + c1) * (T(2) * cab + c2)) / ((mua * mua + mub * mub + c1) * (va + vb + c2))
            total += float(S[:, :min(TILE, H - 10 - y0), :min(TILE, W - 10 - x0)].astype(np.float64).sum())
    return total / (C * (H - 10) * (W - 10))


# ---- the cases -----------------------------------------------------------------------------------------------------------------------

SHAPES = [(1, 11, 11), (3, 11, 75), (3, 75, 11), (3, 37, 53), (3, 70, 90)]
KINDS = ("smooth", "noise", "flat")
PAIRINGS = [("float16", "float16"), ("float16", "float32"), ("float32", "float16"), ("float32", "float32")]


def box_blur(x):
    p = np.pad(x, ((0, 0), (1, 1), (1, 1)), mode="edge")
    H, W = x.shape[1:]
    return sum(p[:, i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0


def image_pair(kind, shape, seed=0):
    """float64 (a, b) in [0, 1]: smooth vs box-blurred, uniform noise vs blurred, a near-flat bright image vs itself plus noise"""
    C, H, W = shape
    rng = np.random.RandomState(1000 * seed + 17 * H + W + C)
    if kind == "smooth":
        i, j = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
        b = np.stack([0.525 + 0.475 * np.sin(0.23 * i + 0.7 * c) * np.cos(0.17 * j - 0.4 * c) for c in range(C)])
        return box_blur(b), b
    if kind == "noise":
        b = rng.uniform(0, 1, size=shape)
        return box_blur(b), b
    b = 0.9 + 1e-3 * rng.uniform(-1, 1, size=shape)
    return b + 1e-3 * rng.uniform(-1, 1, size=shape), b


@functools.lru_cache(maxsize=None)
def case(kind, shape, dt_a="float16", dt_b="float32", seed=0):
    """dict: a, b (numpy, in their dtypes), want = (mse, psnr_db, ssim) in float64 of exactly those values, d = the float32 restatement's
    SSIM deviation, d_half = the same with the shift by L / 2, tol = the SSIM tolerance"""
    a, b = image_pair(kind, shape, seed)
    a, b = a.astype(dt_a), b.astype(dt_b)
    want = ref_quality(a, b)
    d = abs(ref_quality_tiled(a, b) - want[2])
    d_half = abs(ref_quality(a, b, dtype=np.float32, pivot="half")[2] - want[2])
    return dict(a=a, b=b, want=want, d=d, d_half=d_half, tol=max(8 * min(d, d_half), 2.0 ** -20))


def check_against_reference(got, cs, label):
    """got: 3 floats (mse, psnr_db, ssim) of the code under test"""
    mse, psnr, ssim = (float(v) for v in got)
    w_mse, w_psnr, w_ssim = cs["want"]
    print("%s: ssim err %.3g (d %.3g, d_half %.3g, tolerance %.3g), psnr err %.3g dB"
          % (label, abs(ssim - w_ssim), cs["d"], cs.get("d_half", float("nan")), cs["tol"], abs(psnr - w_psnr)))
    assert cs["tol"] <= SSIM_CAP, (label, cs["tol"])
    assert abs(ssim - w_ssim) <= cs["tol"], (label, ssim, w_ssim, cs["tol"])
    assert abs(psnr - w_psnr) <= PSNR_TOL, (label, psnr, w_psnr)
    assert abs(mse - w_mse) <= 1e-5 * w_mse + 1e-12, (label, mse, w_mse)      # fp32 storage of the result: 6e-8 relative


def tensors(cs):
    return torch.from_numpy(cs["a"].copy()), torch.from_numpy(cs["b"].copy())


# ---- 1: the definition -----------------------------------------------------------------------------------------------------------------

def test_window_is_skimages():
    """the moments = scipy.ndimage.gaussian_filter(sigma=1.5, truncate=3.5) cropped by 5 on each side: skimage's own route"""
    ndimage = pytest.importorskip("scipy.ndimage")
    x = image_pair("noise", (2, 31, 40))[1]
    for plane, got in zip(x, ref_moment(x)):
        want = ndimage.gaussian_filter(plane, sigma=1.5, truncate=3.5, mode="reflect")[5:-5, 5:-5]
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12


def test_the_kernels_window_is_the_definitions_to_fp32_rounding():
    """WINDOW: multiples of 2^-24 that sum to exactly 1, each within 2^-25 of the exact weight (the fp32 rounding of the centre tap)"""
    from detectinblur_amd import quality as Q
    g = np.array(Q.WINDOW)
    assert len(g) == 11 and np.array_equal(g, g[::-1]) and np.array_equal(g.astype(np.float32).astype(np.float64), g)
    assert np.array_equal(g * 2 ** 24, np.round(g * 2 ** 24)) and g.sum() == 1.0 and np.float32(0.5) * g.astype(np.float32).sum(dtype=np.float32) == 0.5
    assert np.abs(g - ref_window()).max() <= 2.0 ** -25
    src = open(os.path.join(ROOT, "detectinblur_amd", "csrc", "dib_quality.hip")).read()
    assert all("%d.f / 16777216.f" % v in src for v in Q._WINDOW_2_24)


@pytest.mark.parametrize("dt_a,dt_b", PAIRINGS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_torch_path_against_the_float64_definition(shape, kind, dt_a, dt_b):
    from detectinblur_amd import quality as Q
    cs = case(kind, shape, dt_a, dt_b)
    a, b = tensors(cs)
    got = Q.psnr_ssim(a, b)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3,) and not got.is_cuda
    check_against_reference(got.tolist(), cs, "%s %s %s/%s" % (kind, shape, dt_a, dt_b))


def test_data_range_scales_the_constants():
    from detectinblur_amd import quality as Q
    a, b = image_pair("noise", (3, 37, 53))
    a, b = (255.0 * a).astype(np.float32), (255.0 * b).astype(np.float32)
    want = ref_quality(a, b, L=255.0)
    d = min(abs(ref_quality_tiled(a, b, L=255.0) - want[2]), abs(ref_quality(a, b, L=255.0, dtype=np.float32, pivot="half")[2] - want[2]))
    got = Q.psnr_ssim(torch.from_numpy(a), torch.from_numpy(b), data_range=255.0).tolist()
    assert abs(got[2] - want[2]) <= max(8 * d, 2.0 ** -20) <= SSIM_CAP and abs(got[1] - want[1]) <= PSNR_TOL


# ---- 2: closed forms (tests/test_quality_gpu.py runs the same on the HIP path) -----------------------------------------------------------

def check_closed_forms(fn, device="cpu"):
    """fn(a, b) -> 3-element tensor"""
    g = torch.Generator().manual_seed(3)
    x = torch.rand(3, 37, 53, generator=g).to(device)
    for a, b in ((x, x), (x, x.clone()), (x.half(), x.half().float()), (x.half(), x.half().clone())):
        got = fn(a, b).tolist()
        assert got[0] == 0.0 and got[1] == float("inf") and got[2] == 1.0, got
    z = torch.zeros(2, 20, 45, device=device)
    assert fn(z, z.half()).tolist() == [0.0, float("inf"), 1.0]
    got = fn(z, torch.ones(2, 20, 45, device=device)).tolist()
    c1 = 1e-4
    assert got[0] == 1.0 and got[1] == 0.0 and abs(got[2] - c1 / (1 + c1)) <= 1e-9, got
    y = (0.5 * x + 0.1).clone()
    y[1, 17, 30] = float("nan")
    got = fn(x, y).tolist()
    assert np.isnan(got[0]) and np.isnan(got[2]) and np.isnan(got[1]), got
    got = fn(y.half(), x).tolist()
    assert np.isnan(got[0]) and np.isnan(got[2]), got


def test_closed_forms():
    from detectinblur_amd import quality as Q
    check_closed_forms(Q.psnr_ssim)


def test_psnr_is_the_trainers():
    from detectinblur_amd import quality as Q, train_deblurrer as TD
    for kind in KINDS:
        a, b = tensors(case(kind, (3, 37, 53), "float16", "float32"))
        assert abs(float(Q.psnr_ssim(a, b)[1]) - TD.psnr(a, b)) <= PSNR_TOL


def test_python_argument_checks():
    from detectinblur_amd import quality as Q
    x = torch.rand(3, 20, 30)
    for a, b, msg in ((x[:, :10].contiguous(), x[:, :10].contiguous(), "smaller than the 11 x 11"), (x[:, :, :10].contiguous(), x[:, :, :10].contiguous(), "smaller than"),
                      (x, x[:, :19].contiguous(), "shapes differ"), (x[0], x[0], "planar"), (x[None], x[None], "planar"),
                      (x[:, :, ::2], x[:, :, ::2], "contiguous"), (x.permute(0, 2, 1), x.permute(0, 2, 1), "contiguous")):
        with pytest.raises(ValueError, match=msg):
            Q.psnr_ssim(a, b)
    for L in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="data_range"):
            Q.psnr_ssim(x, x, data_range=L)
    with pytest.raises(TypeError):
        Q.psnr_ssim(x.double(), x)
    out = torch.zeros(3)
    assert Q.psnr_ssim(x, x, out=out) is out and out.tolist() == [0.0, float("inf"), 1.0]
    with pytest.raises(ValueError, match="out must be"):
        Q.psnr_ssim(x, x, out=torch.zeros(4))


# ---- 3: behaviour -----------------------------------------------------------------------------------------------------------------------

def test_richardson_lucy_improves_both_figures_with_its_iterations():
    """the metric on the stage it is for: the "reflect" case of tests/test_deconvolve_first.py (3 x 70 x 90, 42 taps), the blurred image
    and Richardson-Lucy at N = 5 and 30 against the truth.  Measured with the float64 definition: 10.16 dB / -0.261, 17.02 dB / 0.780,
    20.36 dB / 0.909.  The order is asserted, not the values."""
    from detectinblur_amd import quality as Q
    from detectinblur_amd.models import deconvolve as DC
    from tests.test_deconvolve_first import case as rl_case, torch_psf
    cs = rl_case("reflect")
    truth = torch.from_numpy(cs["truth"]).float()
    y = torch.from_numpy(cs["y16"].copy())
    figures = [Q.psnr_ssim(y, truth).tolist()]
    for n in (5, 30):
        figures.append(Q.psnr_ssim(DC.richardson_lucy(y, torch_psf(cs), iterations=n), truth).tolist())
    print("N = 0, 5, 30: (mse, psnr, ssim) =", figures)
    assert figures[0][1] < figures[1][1] < figures[2][1] and figures[0][2] < figures[1][2] < figures[2][2]
    assert figures[0][0] > figures[1][0] > figures[2][0]


# ---- 4: the C entry point ------------------------------------------------------------------------------------------------------------------

def test_entry_point_is_declared_and_bound():
    from detectinblur_amd import _lib
    header = open(os.path.join(ROOT, "include", "dib.h")).read()
    assert re.search(r"\bint dib_image_quality\(", header) and re.search(r"\bsize_t dib_image_quality_workspace_bytes\(", header)
    assert "dib_image_quality" in _lib.EXPORTS and _lib.lib().dib_image_quality is not None
    assert "dib_quality.hip" in open(os.path.join(ROOT, "detectinblur_amd", "csrc", "Makefile")).read()
    l = _lib.lib()
    assert l.dib_image_quality_workspace_bytes(3, 800, 1333) > 0 and l.dib_image_quality_workspace_bytes(3, 800, 1333) % 8 == 0
    assert l.dib_image_quality_workspace_bytes(3, 10, 50) == 0 and l.dib_image_quality_workspace_bytes(0, 20, 50) == 0


def test_argument_errors_are_reported_without_a_gpu():
    """every refusal launches nothing and touches no pointer: the addresses below are never dereferenced"""
    from detectinblur_amd import _lib
    l = _lib.lib()
    A, B, OUT, WORK = 1 << 20, 2 << 20, 3 << 20, 4 << 20

    def call(a=A, adt=_lib.DIB_F16, b=B, bdt=_lib.DIB_F32, C=3, H=70, W=90, L=1.0, out=OUT, work=WORK):
        return l.dib_image_quality(a, adt, b, bdt, C, H, W, L, out, work, None)
    E, S = _lib.DIB_EINVAL, _lib.DIB_ESHAPE
    for kw in (dict(a=None), dict(b=None), dict(out=None), dict(work=None)):
        assert call(**kw) == E and b"null pointer" in l.dib_last_error(), kw
    for kw in (dict(adt=2), dict(bdt=-1)):
        assert call(**kw) == E and b"dtype" in l.dib_last_error(), kw
    for kw in (dict(C=0), dict(H=0), dict(W=-2)):
        assert call(**kw) == E and b"empty shape" in l.dib_last_error(), kw
    for L in (0.0, -1.0, float("inf"), float("nan")):
        assert call(L=L) == E and b"data_range" in l.dib_last_error(), L
    for kw in (dict(H=10), dict(W=10), dict(H=1, W=1)):
        assert call(**kw) == S and b"smaller than the 11 x 11 window" in l.dib_last_error(), kw
    assert call(C=1 << 15, H=1 << 8, W=1 << 8) == S and b"too large" in l.dib_last_error()
    for kw in (dict(a=A + 1), dict(b=B + 2), dict(out=OUT + 2), dict(work=WORK + 4)):
        assert call(**kw) == E and b"misaligned" in l.dib_last_error(), kw
    n = 3 * 70 * 90
    for kw in (dict(out=A), dict(out=A + 2 * n - 4), dict(out=B + 4 * n - 4), dict(work=B + 8), dict(work=A - 8), dict(out=WORK + 8)):
        assert call(**kw) == E and b"overlap" in l.dib_last_error(), kw


# ---- 5: the trainer ----------------------------------------------------------------------------------------------------------------------------

def test_deblurrer_validation_prints_the_ssim_pair_beside_the_psnr(tmp_path):
    from detectinblur_amd import train_deblurrer as TD
    from tests.test_deblur_train import TINY
    argv = ["--synthetic", "--synthetic_images", "4", "--synthetic_size", "40", "56", "--device", "cpu", "-j", "0", "-b", "2", "--patch_size", "16",
            "--print_freq", "1", "--output_dir", str(tmp_path), "--epochs", "1", "--early_stop", "0", "--validate_images", "2"] + TINY
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        TD.main(argv)
    m = re.search(r"Validation: \[1\]  PSNR deblurred (\S+) dB, blurred input (\S+) dB; SSIM deblurred (\S+), blurred input (\S+) \(2 images, SSIM over 2 of them; no quality claim\)",
                  buf.getvalue())
    assert m, buf.getvalue()[-600:]
    assert all(np.isfinite(float(v)) for v in m.groups()) and -1 <= float(m.group(3)) <= 1 and -1 <= float(m.group(4)) <= 1
