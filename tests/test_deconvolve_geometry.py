"""The Richardson-Lucy sweeps (csrc/dib_deconv.hip, models/deconvolve.py) on the data and shapes the cases of
tests/test_deconvolve_first.py do not reach: white noise with exact zeros and ones (every tap coordinate matters at full amplitude,
both clamp ends are taken), a PSF with taps in the canvas corners (offsets -63..+64 / -127..+128: the second reflection branch, the
far side of the clamp), images of whole tiles, images thinner than a tile or a wave, one pixel, images far smaller than the tap
offsets on the 256 canvas, C = 5, and an eps large enough to be taken on half of an image.  This module is the host side: the
inputs, the conditions that say each case still probes what it is for (from the float64 reference alone), a table showing that the
reference tells nine deliberate errors apart on these cases, and the torch restatement (the `--device cpu` path) against float64.
tests/test_deconvolve_geometry_gpu.py puts the same cases through the HIP kernels.

The float64 definition (ref_map, ref_sweep, ref_rl), trace_psf, dense_psf and the tolerance rule max(8 d, N 2^-20) (reference_of) are
those of tests/test_deconvolve_first.py, imported."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from tests.test_deconvolve_first import EPS, dense_psf, ref_map, ref_mode, ref_sweep, reference_of, trace_psf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


# ---- 1: the inputs ---------------------------------------------------------------------------------------------------------------------

def noisy(C, H, W, seed, dtype=np.float16):
    """white noise in [0, 1) with 10 % exact zeros and 5 % exact ones, rounded to `dtype` (Half: what the blur hands on)"""
    rs = np.random.RandomState(seed)
    y = rs.random_sample((C, H, W))
    m = rs.random_sample((C, H, W))
    y[m < 0.10] = 0
    y[m > 0.95] = 1
    return y.astype(dtype)


def far_psf(K):
    """trace_psf (wrap taps included) plus taps in three corners of the canvas, next to the fourth and in row 1: the largest offsets
    of either sign in rows and in columns.  All values stay small multiples of 2^-10: the sum is exact in Half in any order."""
    psf = trace_psf(K)
    for (r, c), v in zip(((0, 0), (0, K - 1), (K - 1, 0), (K - 2, K - 2), (1, K // 2)), (4, 1, 5, 2, 3)):
        assert psf[r, c] == 0
        psf[r, c] = v / 1024.0
    return psf


def far_psf_scaled(K):
    """far_psf times 3: other Half bits, the same normalised weights up to rounding (a fourth, different table of one TapTables)"""
    return 3 * far_psf(K)


PSFS = {"far": far_psf, "trace": trace_psf, "dense": dense_psf, "far3": far_psf_scaled}

# name -> (C, H, W, K, seed of noisy: the case's position): all with far_psf, N in MATRIX_N
MATRIX = {
    "tiles_exact": (1, 96, 128, 128, 1),          # 3 x 2 whole tiles, reflect
    "reflect_min_wide": (1, 65, 300, 128, 2),     # the smallest reflect height, 5 tile columns
    "reflect_planes": (2, 70, 90, 128, 3),        # the shape of test_deconvolve_first.py on hard data
    "zero_thin_rows": (1, 3, 200, 128, 4),        # zero padding, 3 rows
    "zero_thin_cols": (1, 200, 3, 128, 5),        # zero padding, 3 columns
    "zero_tile": (1, 32, 64, 128, 6),             # exactly one tile; W = 64 is legal because H < 64
    "one_pixel": (1, 1, 1, 128, 7),               # the reference gives 0
    "replicate_tiny": (3, 5, 7, 256, 8),          # an image far smaller than the tap offsets
    "replicate_64": (1, 64, 64, 256, 9),          # a side of 64 is legal on the 256 canvas
    "replicate_planes": (5, 33, 129, 256, 10),    # C = 5, one column past two tiles
}
MATRIX_N = (1, 2)
# the data regimes, on 2 x 70 x 90 with trace_psf(128): name -> (eps, iterations)
REGIMES = {"eps_large": (0.25, (1, 2)), "clamp": (EPS, (1, 2, 5))}
# (case, N) of everything below and in the GPU module
RUNS = [(name, n) for name in MATRIX for n in MATRIX_N] + [(name, n) for name in REGIMES for n in REGIMES[name][1]]
F32_CASES = ("tiles_exact", "zero_thin_cols", "replicate_tiny")      # also with an fp32 image and an fp32 table


@functools.lru_cache(maxsize=None)
def taps_for(psf_name, K, psf_dtype="float16"):
    """(the un-normalised PSF in psf_dtype, (rows, cols, float64 weights of the PSF normalised in its own dtype, row-major))"""
    import dib_oracle as O
    psf = PSFS[psf_name](K)
    psf = O.to_half_like_torch(psf) if psf_dtype == "float16" else psf.astype(np.float32)
    rows, cols, wts = O.taps_of(O.normalize_psf(psf))
    return psf, (rows, cols, wts.astype(np.float64))


@functools.lru_cache(maxsize=None)
def case(name, y_dtype="float16", psf_dtype="float16", psf_name=None):
    """dict: y (the image in y_dtype), psf (K x K in psf_dtype, un-normalised), taps, K, shape, eps.  psf_name replaces the case's PSF
    (the large-window and table-index tests)."""
    if name in MATRIX:
        C, H, W, K, seed = MATRIX[name]
        y, eps, own = noisy(C, H, W, seed, np.dtype(y_dtype).type), EPS, "far"
    else:
        (C, H, W, K), eps, own = (2, 70, 90, 128), REGIMES[name][0], "trace"
        if name == "eps_large":      # A y lies below eps on the dim half, above it on the bright half
            rs = np.random.RandomState(3)
            y = (rs.random_sample((C, H, W)) * np.where(np.arange(W) < 45, 0.3, 1.0)).astype(y_dtype)
        else:
            y = noisy(C, H, W, 1, np.dtype(y_dtype).type)
    psf, taps = taps_for(psf_name or own, K, psf_dtype)
    return dict(y=y, psf=psf, taps=taps, K=K, shape=(C, H, W), eps=eps)


@functools.lru_cache(maxsize=None)
def reference(name, iterations, y_dtype="float16", psf_dtype="float16", psf_name=None):
    """(x_N in float64, tolerance, d) of a case: computed once, shared by both modules, never written to"""
    cs = case(name, y_dtype, psf_dtype, psf_name)
    want, tol, d = reference_of(cs["y"], cs["taps"], cs["K"], iterations, cs["eps"])
    want.setflags(write=False)
    return want, tol, d


def test_inputs_are_what_they_say():
    y = noisy(2, 70, 90, 1)
    assert y.dtype == np.float16 and y.min() == 0 and y.max() == 1
    assert 0.08 < (y == 0).mean() < 0.12 and 0.03 < (y == 1).mean() < 0.07
    for K in (128, 256):
        psf, (rows, cols, wts) = taps_for("far", K)
        assert len(rows) == 47 and psf.dtype == np.float16
        # exact in Half: every value a small multiple of 2^-10, the sum below 2048 of them
        assert np.array_equal(psf.astype(np.float64), far_psf(K)) and float(far_psf(K).sum() * 1024) == round(far_psf(K).sum() * 1024) < 2048
        o = K // 2 - 1
        assert (rows - o).min() == -o and (rows - o).max() == K // 2 and (cols - o).min() == -o and (cols - o).max() == K // 2
    assert [ref_mode(K, H, W) for (_, H, W, K, _) in MATRIX.values()] == ["reflect"] * 3 + ["zero"] * 4 + ["replicate"] * 3
    assert len({seed for (_, _, _, _, seed) in MATRIX.values()}) == len(MATRIX)


def test_conditions_each_case_still_probes_what_it_is_for():
    """from the float64 reference alone"""
    for name in MATRIX:
        for n in MATRIX_N:
            want, _, _ = reference(name, n)
            if name == "one_pixel":
                assert case(name)["y"].item() > 0 and want.shape == (1, 1, 1) and want.item() == 0
                continue
            inside = float(((want > 0.02) & (want < 0.98)).mean())
            print("%-17s N=%d: %.2f of the reference strictly inside (0.02, 0.98)" % (name, n, inside))
            assert inside >= 0.60, (name, n, inside)
    want, _, _ = reference("clamp", 1)
    ones, zeros = float((want == 1).mean()), float((want == 0).mean())
    print("clamp N=1: %.3f of the reference == 1, %.3f == 0" % (ones, zeros))
    assert ones >= 0.03 and zeros >= 0.05
    cs = case("eps_large")
    ay = ref_sweep(cs["y"].astype(np.float64), cs["taps"], cs["K"], False)
    below, above = float((ay < cs["eps"]).mean()), float((ay > cs["eps"]).mean())
    print("eps_large: A y < eps on %.2f of the pixels, > eps on %.2f" % (below, above))
    assert below >= 0.25 and above >= 0.25
    for name in ("zero_thin_rows", "zero_thin_cols"):      # the eps branch taken with a huge quotient
        cs = case(name)
        y = cs["y"].astype(np.float64)
        huge = float(((y > 0) & (ref_sweep(y, cs["taps"], cs["K"], False) < 1e-6)).mean())
        print("%s: y > 0 and A y < 1e-6 on %.4f of the pixels" % (name, huge))
        assert huge > 0
    worst = 0.0
    for name, n in RUNS:
        _, tol, d = reference(name, n)
        worst = max(worst, d)
        assert d < 1e-6, (name, n, d)
    for name in F32_CASES:
        for n in MATRIX_N:
            d = reference(name, n, "float32", "float32")[2]
            worst = max(worst, d)
            assert d < 1e-6, (name, n, d)
    print("largest float32 restatement deviation d over all cases: %.3g" % worst)


# ---- 2: the reference can tell -----------------------------------------------------------------------------------------------------------

VARIANTS = ("adjoint_sign", "swapped", "reflect_edge", "zero_as_replicate", "no_wrap", "centre", "plus_eps", "eps_fixed", "no_clamp")


def variant_rl(y, taps, K, iterations, eps=EPS, error=None):
    """the float64 definition with one deliberate error (None: the definition itself, equal to ref_rl bit for bit):
    adjoint_sign: A* with A's offset sign;  swapped: row and column offsets exchanged;  reflect_edge: reflection that repeats the edge;
    zero_as_replicate: zero padding read as replicate;  no_wrap: A without the wrap row / column;  centre: o = K / 2;
    plus_eps: y / (A x + eps);  eps_fixed: eps = 1e-6 whatever is passed;  no_clamp: no upper clamp"""
    assert error is None or error in VARIANTS
    rows, cols, weights = taps
    if error == "swapped":
        rows, cols = cols, rows
    y = np.asarray(y).astype(np.float64)
    C, H, W = y.shape
    o = K // 2 if error == "centre" else K // 2 - 1
    mode = ref_mode(K, H, W)
    if error == "zero_as_replicate" and mode == "zero":
        mode = "replicate"
    if error == "eps_fixed":
        eps = 1e-6

    def coord(s, n, wrap):
        if error == "reflect_edge" and mode == "reflect":
            s = np.asarray(s, dtype=np.int64).copy()
            if wrap:
                s[s == -(K // 2)] = n + K // 2 - 1
            s = np.where(s < 0, -s - 1, s)
            s = np.where(s > n - 1, 2 * n - 1 - s, s)
            return np.clip(s, 0, n - 1), np.zeros(s.shape, dtype=bool)
        return ref_map(s, n, K, mode, wrap)

    def sweep(x, adjoint):
        plus = adjoint and error != "adjoint_sign"
        wrap = not adjoint and error != "no_wrap"
        acc = np.zeros((C, H, W), dtype=np.float64)
        i, j = np.arange(H), np.arange(W)
        for r, c, w in zip(rows, cols, weights):
            si, zi = coord(i + (r - o) if plus else i - (r - o), H, wrap)
            sj, zj = coord(j + (c - o) if plus else j - (c - o), W, wrap)
            g = x[:, si][:, :, sj]
            if mode == "zero":
                g = g * (~zi[None, :, None] & ~zj[None, None, :]).astype(np.float64)
            acc = acc + np.float64(w) * g
        return acc

    x = y
    for _ in range(iterations):
        ax = sweep(x, False)
        q = y / (ax + eps if error == "plus_eps" else np.maximum(ax, np.float64(eps)))
        x = np.maximum(x * sweep(q, True), 0.0) if error == "no_clamp" else np.clip(x * sweep(q, True), 0.0, 1.0)
    return x


def test_the_variant_runner_without_an_error_is_the_definition():
    for name, n in RUNS:
        cs = case(name)
        assert np.array_equal(variant_rl(cs["y"], cs["taps"], cs["K"], n, cs["eps"]), reference(name, n)[0]), (name, n)


def test_the_reference_tells_each_deliberate_error_apart():
    """deviation / tolerance of every variant on every case at N = 1: each variant is off by more than 100 tolerances somewhere (0:
    the variant is a no-op on that case -- the wrap under zero padding, the reflection on the 256 canvas)"""
    names = list(MATRIX) + list(REGIMES)
    table = np.zeros((len(names), len(VARIANTS)))
    for a, name in enumerate(names):
        cs = case(name)
        want, tol, _ = reference(name, 1)
        for b, error in enumerate(VARIANTS):
            table[a, b] = np.abs(variant_rl(cs["y"], cs["taps"], cs["K"], 1, cs["eps"], error) - want).max() / tol
    print("deviation from the float64 definition / tolerance, N = 1")
    print("%-17s" % "case" + "".join("%18s" % v for v in VARIANTS))
    for a, name in enumerate(names):
        print("%-17s" % name + "".join("%18.3g" % v for v in table[a]))
    for b, error in enumerate(VARIANTS):
        assert table[:, b].max() > 100, (error, table[:, b])


# ---- 3: the torch restatement ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,iterations", RUNS, ids=["%s-%d" % r for r in RUNS])
def test_torch_path_against_the_float64_definition(name, iterations):
    from detectinblur_amd.models import deconvolve as DC
    cs = case(name)
    want, tol, d = reference(name, iterations)
    got = DC.richardson_lucy(torch.from_numpy(cs["y"].copy()), torch.from_numpy(cs["psf"].copy()), iterations=iterations, eps=cs["eps"])
    assert got.dtype == torch.float32 and tuple(got.shape) == cs["shape"] and not got.is_cuda
    err = float(np.abs(got.numpy().astype(np.float64) - want).max())
    print("%s N=%d: torch vs float64 %.3g, float32 restatement %.3g, tolerance %.3g" % (name, iterations, err, d, tol))
    assert err <= tol, (err, tol)
