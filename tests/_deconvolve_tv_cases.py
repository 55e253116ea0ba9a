"""The float64 statement of total-variation regularised Richardson-Lucy (include/dib.h: dib_tv_weight, dib_rl_deconvolve_tv), stated once
for tests/test_deconvolve_tv.py (host) and tests/test_deconvolve_tv_gpu.py (the HIP kernel and stage), on top of the sweeps, cases and
tolerance rule of tests/test_deconvolve_first.py.

Per plane x of H x W, with beta > 0 and 0 < lambda <= 0.1:
    dx[i, j] = x[i, j + 1] - x[i, j]   (0 where j == W - 1)         dy[i, j] = x[i + 1, j] - x[i, j]   (0 where i == H - 1)
    n = sqrt(dx^2 + dy^2 + beta^2)      p = dx / n      r = dy / n
    div[i, j] = (p[i, j] - p[i, j - 1]) + (r[i, j] - r[i - 1, j])    with p[i, -1] = 0 and r[-1, j] = 0
    g = 1 / (1 - lambda div)            tv_weight(x) = x * g
    q = y / max(A x_k, eps);   x_{k+1} = clamp((x_k * g_k) * (A* q), 0, 1);   x_0 = y

Tolerance of every comparison against float64: the rule of tests/test_deconvolve_first.py, max(8 d, N 2^-20), with d the largest deviation
from float64 of a float32 numpy restatement of the same case, computed here at run time from the reference alone (N = 1 for the factor
on its own).  So that the rule cannot hide a failure, d <= 2^-12 is asserted before the tolerance is used: with beta = 1e-2 and
lambda <= 0.01 the float32 restatement stays below 1e-4 even at N = 30 (with beta = 1e-3 it drifts to 2e-2: dx / n loses its
conditioning on near-flat regions, which is why the default beta and the values used here are 1e-2)."""
import functools

import numpy as np

from tests.test_deconvolve_first import EPS, case, ref_sweep

BETA = 1e-2
LAMBDAS = (0.002, 0.01)
ITERATIONS = (1, 2, 5)
D_MAX = 2.0 ** -12


def ref_tv_weight(x, lam, beta, dtype=np.float64):
    """x * g of planes C x H x W in `dtype`, straight from the definition"""
    x = np.asarray(x).astype(dtype)
    lam, beta = dtype(lam), dtype(beta)
    dx, dy = np.zeros_like(x), np.zeros_like(x)
    dx[:, :, :-1] = x[:, :, 1:] - x[:, :, :-1]
    dy[:, :-1, :] = x[:, 1:, :] - x[:, :-1, :]
    n = np.sqrt(dx * dx + dy * dy + beta * beta)
    p, r = dx / n, dy / n
    p_left, r_up = np.zeros_like(x), np.zeros_like(x)
    p_left[:, :, 1:] = p[:, :, :-1]
    r_up[:, 1:, :] = r[:, :-1, :]
    div = (p - p_left) + (r - r_up)
    out = x * (dtype(1) / (dtype(1) - lam * div))
    assert out.dtype == dtype
    return out


def ref_rl_tv(y, taps, K, iterations, lam, beta, eps=EPS, dtype=np.float64):
    y = np.asarray(y).astype(dtype)
    x = y
    for _ in range(iterations):
        q = y / np.maximum(ref_sweep(x, taps, K, False, dtype), dtype(eps))
        x = np.clip(ref_tv_weight(x, lam, beta, dtype) * ref_sweep(q, taps, K, True, dtype), dtype(0), dtype(1))
    return x


def _tolerance(want, restated, iterations):
    d = float(np.abs(restated.astype(np.float64) - want).max())
    assert d <= D_MAX, "the float32 restatement itself is %.3g from float64: the tolerance rule would hide a failure" % d
    return max(8 * d, iterations * 2.0 ** -20), d


def reference_tv_weight_of(x, lam, beta=BETA):
    """(x * g in float64, tolerance, d) of planes x (Half or fp32 values)"""
    want = ref_tv_weight(x, lam, beta)
    tol, d = _tolerance(want, ref_tv_weight(x, lam, beta, np.float32), 1)
    return want, tol, d


def reference_tv_of(y, taps, K, iterations, lam, beta=BETA, eps=EPS):
    """(x_N in float64, tolerance, d) of one image and tap list"""
    want = ref_rl_tv(y, taps, K, iterations, lam, beta, eps)
    tol, d = _tolerance(want, ref_rl_tv(y, taps, K, iterations, lam, beta, eps, np.float32), iterations)
    return want, tol, d


def image_np(name, y_dtype="float16"):
    """the blurred image of a case of tests/test_deconvolve_first.py: the Half one, or the fp32 rounding of the same float64 blur"""
    cs = case(name)
    return cs["y16"] if y_dtype == "float16" else ref_sweep(cs["truth"], cs["taps"], cs["K"], False).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference_tv(name, iterations, lam, y_dtype="float16"):
    cs = case(name)
    return reference_tv_of(image_np(name, y_dtype), cs["taps"], cs["K"], iterations, lam)


# ---- the factor on its own ---------------------------------------------------------------------------------------------------------------

# H x W: a single pixel, a single row, a single column, the smallest plane with all four edges, one pixel over the kernel's tile of
# 62 x 32 on both sides (63 x 33) and one over 64 x 32 (65 x 33), several tiles with ragged edges (90 x 70: columns 62.. and rows
# 64.. in a second / third tile)
KERNEL_SHAPES = ((1, 1), (1, 67), (67, 1), (2, 2), (33, 63), (33, 65), (70, 90))
PLANE_LEVELS = (0.1, 0.9, 0.5)


@functools.lru_cache(maxsize=None)
def plane_set(C, H, W, dtype="float32"):
    """C planes at very different levels (0.1 / 0.9 / 0.5) plus noise of 0.05: a stencil that runs from one plane's last row into the
    next plane's first, or wraps from a row's end into the next row, sees a jump of up to 0.8 where the definition has a difference of 0"""
    rs = np.random.RandomState(1000 * C + 10 * H + W)
    x = np.stack([PLANE_LEVELS[c % 3] + 0.05 * rs.standard_normal((H, W)) for c in range(C)])
    x = np.clip(x, 0, 1).astype(np.float16 if dtype == "float16" else np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference_tv_weight(C, H, W, dtype, lam):
    return reference_tv_weight_of(plane_set(C, H, W, dtype), lam)


# ---- the behavioural case -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def block_case(sigma=0.03):
    """case `reflect` (3 x 70 x 90, the 42-tap trace) with a piecewise-constant truth -- blocks of 10 rows x 15 columns at levels k / 8 --
    blurred, plus Gaussian noise of `sigma`, clipped to [0, 1] and rounded to Half: dict(truth, y16, taps, K)"""
    cs = case("reflect")
    C, H, W = cs["shape"]
    rs = np.random.RandomState(7)
    levels = rs.randint(0, 9, size=(C, H // 10, W // 15)) / 8.0
    truth = np.kron(levels, np.ones((1, 10, 15)))
    assert truth.shape == (C, H, W)
    y = ref_sweep(truth, cs["taps"], cs["K"], False) + sigma * rs.standard_normal((C, H, W))
    return dict(truth=truth, y16=np.clip(y, 0, 1).astype(np.float16), taps=cs["taps"], K=cs["K"], psf=cs["psf"])


def total_variation(x):
    """sum over all pixels of |grad x| (forward differences, 0 past the last row / column)"""
    x = np.asarray(x, dtype=np.float64)
    dx, dy = np.zeros_like(x), np.zeros_like(x)
    dx[:, :, :-1] = np.diff(x, axis=2)
    dy[:, :-1, :] = np.diff(x, axis=1)
    return float(np.sqrt(dx * dx + dy * dy).sum())


def mse(x, truth):
    return float(((np.asarray(x, dtype=np.float64) - truth) ** 2).mean())
