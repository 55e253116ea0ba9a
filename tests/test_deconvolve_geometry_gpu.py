"""The two sweep kernels of csrc/dib_deconv.hip (dib_rl_deconvolve) on the cases of tests/test_deconvolve_geometry.py -- whole tiles,
images thinner than a tile, one pixel, images smaller than the tap offsets, C = 5, taps in the canvas corners, white noise with exact
zeros and ones, a large eps -- against the float64 definition with the tolerance rule max(8 d, N 2^-20) of
tests/test_deconvolve_first.py; tables compacted for the large LDS window whose boxes the kernel has to cut in both directions; the
raw entry point on a NaN-filled output and workspace; images at odd addresses; and every table of a TapTables of four PSFs."""
import numpy as np
import pytest
import torch

from tests.test_deconvolve_geometry import F32_CASES, MATRIX_N, RUNS, case, reference

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEG_ROWS, SEG_COLS = 13, 25      # the standard window's box (csrc/dib_common.h: SEG_ROWS + 1, SEG_COLS + 1): what the kernel cuts larger boxes into


def tables_of(*cases, **kw):
    from detectinblur_amd import blur_ops
    return blur_ops.compact_psfs([torch.from_numpy(cs["psf"].copy()).to(DEV) for cs in cases], normalize=True, **kw)


def image_of(cs):
    return torch.from_numpy(cs["y"].copy()).to(DEV)


def deviation(got, want):
    return float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())


# ---- 4: every case through the wrapper -------------------------------------------------------------------------------------------------

COMBOS = [(name, n, "float16") for name, n in RUNS] + [(name, n, "float32") for name in F32_CASES for n in MATRIX_N]


@pytest.mark.parametrize("name,iterations,dtype", COMBOS, ids=["%s-%d-%s" % c for c in COMBOS])
def test_hip_against_the_float64_definition(name, iterations, dtype):
    """dtype: of the image and of the PSF table alike (Half: the drivers' types)"""
    from detectinblur_amd.models import deconvolve as DC
    cs = case(name, dtype, dtype)
    want, tol, d = reference(name, iterations, dtype, dtype)
    tables, y = tables_of(cs), image_of(cs)
    assert tables.dtype == getattr(torch, dtype) == y.dtype
    got = DC.richardson_lucy(y, tables, iterations=iterations, eps=cs["eps"])
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == cs["shape"] and bool(torch.isfinite(got).all())
    err = deviation(got, want)
    ref = DC.richardson_lucy_torch(y, DC.taps_of_table(tables, 0), iterations=iterations, eps=cs["eps"])
    print("%s %s N=%d: HIP vs float64 %.3g, float32 restatement %.3g, tolerance %.3g; %d of %d elements differ from the torch path on the device"
          % (name, dtype, iterations, err, d, tol, int((got != ref).sum()), got.numel()))
    assert err <= tol, (err, tol)
    assert torch.equal(got, DC.richardson_lucy(y, tables, iterations=iterations, eps=cs["eps"]))      # deterministic


# ---- 5: the large window, cut both ways ------------------------------------------------------------------------------------------------

# (case, PSF): far_psf and dense_psf on either canvas.  Only the dense PSFs have a box tall enough for the row cut: far_psf's trace is
# cut by its own wrap tap in column K - 1 first
LARGE = [("tiles_exact", "far"), ("tiles_exact", "dense"), ("reflect_planes", "far"), ("reflect_planes", "dense"),
         ("replicate_planes", "far"), ("replicate_planes", "dense")]
LARGE_N = 2


@pytest.mark.parametrize("name,psf_name", LARGE, ids=["%s-%s" % c for c in LARGE])
def test_large_window_tables_are_cut_in_rows_and_in_columns(name, psf_name):
    from detectinblur_amd.models import deconvolve as DC
    cs = case(name, psf_name=psf_name)
    tables = tables_of(cs, large_window=True)
    assert tables.large
    boxes = [(r1 - r0 + 1, c1 - c0 + 1) for (_, _, r0, r1, c0, c1) in tables.segments(0)]
    tall, wide = max(b[0] for b in boxes), max(b[1] for b in boxes)
    want, tol, d = reference(name, LARGE_N, psf_name=psf_name)
    err = deviation(DC.richardson_lucy(image_of(cs), tables, iterations=LARGE_N, eps=cs["eps"]), want)
    print("%s, %s PSF on the %d canvas, large window: %d segments, tallest box %d rows, widest %d columns; N=%d: HIP vs float64 %.3g, float32 "
          "restatement %.3g, tolerance %.3g" % (name, psf_name, cs["K"], len(boxes), tall, wide, LARGE_N, err, d, tol))
    assert wide > SEG_COLS and tall <= 21 and wide <= 64           # `for clo` runs more than once
    if psf_name == "dense":
        assert tall > SEG_ROWS                                     # and so does `for rlo`
    assert err <= tol, (err, tol)


# ---- 6: poisoned buffers through the raw entry point -----------------------------------------------------------------------------------

def raw_call(y, tables, index, iterations, eps):
    """dib_rl_deconvolve itself, on an output and a workspace that hold NaN everywhere"""
    from detectinblur_amd import _lib as L, blur_ops
    C, H, W = (int(v) for v in y.shape)
    out = torch.full((C, H, W), float("nan"), dtype=torch.float32, device=DEV)
    work = torch.full((2, C, H, W), float("nan"), dtype=torch.float32, device=DEV)
    L.check(L.lib().dib_rl_deconvolve(y.data_ptr(), blur_ops._DT[y.dtype], out.data_ptr(), work.data_ptr(), C, H, W, tables.ptr(index),
                                      blur_ops._DT[tables.dtype], tables.K, iterations, eps, L.stream_of(y)))
    return out


@pytest.mark.parametrize("name", ["zero_thin_rows", "tiles_exact", "replicate_tiny"])
def test_no_sweep_reads_what_none_wrote(name):
    """N = 1, 2, 3: both parities of the ping-pong between `out` and the spare plane, and the plane x_0 never occupies"""
    from detectinblur_amd.models import deconvolve as DC
    cs = case(name)
    tables, y = tables_of(cs), image_of(cs)
    for n in (1, 2, 3):
        want, tol, _ = reference(name, n)
        wrapped = DC.richardson_lucy(y, tables, iterations=n, eps=cs["eps"])
        assert deviation(wrapped, want) <= tol
        raw = raw_call(y, tables, 0, n, cs["eps"])
        assert bool(torch.isfinite(raw).all()), n
        assert torch.equal(raw, wrapped), n


# ---- 7: pointers and tables ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,dtype,misalignment", [("reflect_planes", "float16", (4, 2)), ("tiles_exact", "float32", (16, 4))],
                         ids=["half_one_element_in", "float_4_bytes_off_16"])
def test_image_at_an_odd_address(name, dtype, misalignment):
    from detectinblur_amd.models import deconvolve as DC
    cs = case(name, dtype, dtype)
    tables, y = tables_of(cs), image_of(cs)
    buf = torch.zeros(y.numel() + 1, dtype=y.dtype, device=DEV)
    shifted = buf[1:].view(y.shape)
    shifted.copy_(y)
    assert y.data_ptr() % 16 == 0 and shifted.data_ptr() % misalignment[0] == misalignment[1] and shifted.is_contiguous()
    for n in MATRIX_N:
        assert torch.equal(DC.richardson_lucy(shifted, tables, iterations=n, eps=cs["eps"]), DC.richardson_lucy(y, tables, iterations=n, eps=cs["eps"]))


def test_every_table_of_a_batch_is_served():
    """four different PSFs in one TapTables: each index gives the bits of that PSF compacted alone, and stays within the tolerance of
    the float64 definition with that PSF's taps"""
    from detectinblur_amd.models import deconvolve as DC
    name, n = "reflect_planes", 2
    order = ("trace", "far", "dense", "far3")
    cases = [case(name, psf_name=p) for p in order]
    assert all(not np.array_equal(a["psf"], b["psf"]) for i, a in enumerate(cases) for b in cases[:i])
    y = image_of(cases[0])
    batch = tables_of(*cases)
    assert batch.count == 4
    results = []
    for index in (1, 2, 3):
        cs = cases[index]
        got = DC.richardson_lucy(y, (batch, index), iterations=n, eps=cs["eps"])
        assert torch.equal(got, DC.richardson_lucy(y, tables_of(cs), iterations=n, eps=cs["eps"])), order[index]
        want, tol, d = reference(name, n, psf_name=order[index])
        err = deviation(got, want)
        print("%s, table %d (%s) N=%d: HIP vs float64 %.3g, float32 restatement %.3g, tolerance %.3g" % (name, index, order[index], n, err, d, tol))
        assert err <= tol, (order[index], err, tol)
        results.append(got)
    # far and dense differ; far3 normalises to far's very weights (3 v / 3 s), so its result is far's
    assert not torch.equal(results[0], results[1]) and torch.equal(results[0], results[2])
    with pytest.raises(ValueError, match="index 4 out of range"):
        DC.richardson_lucy(y, (batch, 4), iterations=n)
