"""The rasteriser's edge cases (tests/_raster_cases.py) on the CPU: the cases have the properties their names claim, the native host
classes match the oracle on them bit for bit, and a host trajectory that leaves the canvas is refused before any upload.  The device
kernels meet the same cases in tests/test_raster_edges_gpu.py."""
import math
import types

import numpy as np
import pytest
import torch

import dib_oracle as O
from tests import _raster_cases as RC

IN_CANVAS = RC.in_canvas_cases()
HIGH = RC.high_border_cases()
BATCHES = RC.batch_cases()


def _ids(cases):
    return [c[0] for c in cases]


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_case_names_are_unique_and_every_family_is_there():
    names = _ids(IN_CANVAS) + _ids(HIGH) + _ids(BATCHES)
    assert len(set(names)) == len(names)
    for canvas in RC.CANVASES:
        for family in ("random", "single", "lattice", "truncation", "border"):
            assert any(n.startswith("%s_c%d" % (family, canvas)) for n in names), (family, canvas)
        assert sum(n.startswith("high_c%d_" % canvas) for n in names) == 10
    assert sum(n.startswith("exposure_c64_i300") for n in names) == len(RC.FRACTIONS_300) == 9
    assert sum(n.startswith("exposure_c256_i2000") for n in names) == 3
    assert [(c[1], c[2].shape[1], c[2].shape[0]) for c in BATCHES] == [(64, 300, 64), (64, 300, 65), (64, 300, 130), (256, 257, 65)]
    assert sorted({len(c[2]) for c in RC.random_cases()}) == [1, 2, 5, 255, 256, 257, 700]


@pytest.mark.parametrize("case", IN_CANVAS, ids=_ids(IN_CANVAS))
def test_in_canvas_cases_stay_inside(case):
    """1 <= floor(coord) < canvas - 1 for every sample.  The `low` border cases are the stated exception on the low side: they are
    there for coordinates below 1, which the reference clamps to cell 1, and must have some on both axes."""
    name, canvas, re, im, _ = case
    fr, fi = np.floor(re), np.floor(im)
    assert np.all(fr < canvas - 1) and np.all(fi < canvas - 1)
    if RC.is_low_border(name):
        assert (fr < 1).any() and (fi < 1).any() and (re < 0).any() and (im < 0).any()
    else:
        assert np.all(fr >= 1) and np.all(fi >= 1)


def test_in_canvas_batches_stay_inside_and_differ():
    for case in BATCHES:
        name, canvas, traj, fracs = case
        v = traj.view(np.float64)
        assert np.all(np.floor(v) >= 1) and np.all(np.floor(v) < canvas - 1)
        assert len(set(fracs)) == len(fracs)
        raw, cen = RC.expected_batch(case)
        B = len(fracs)
        for b in range(B - 1):
            assert not np.array_equal(raw[b], raw[b + 1]) and not np.array_equal(cen[b], cen[b + 1])
        for b in range(B - 64):
            assert not np.array_equal(raw[b], raw[b + 64]) and not np.array_equal(cen[b], cen[b + 64])


@pytest.mark.parametrize("case", RC.lattice_cases(), ids=_ids(RC.lattice_cases()))
def test_lattice_cases_have_the_stated_count_and_offset_signs(case):
    name, canvas, re, im, frac = case
    n = RC.lattice_count(name)
    raw, _ = RC.expected(case)
    assert len(re) == n + 1 and O.sample_weight(0, frac, 0, len(re)) == 0
    assert int(np.count_nonzero(raw)) == n and int(np.count_nonzero(raw > 0)) == n
    ox, oy = O.psf_center_offsets(raw)
    if name.endswith("_ul"):
        assert ox < 0 and oy < 0
    else:
        assert ox > 0 and oy > 0


@pytest.mark.parametrize("case", RC.truncation_cases(), ids=_ids(RC.truncation_cases()))
def test_truncation_cases_separate_truncation_from_floor(case):
    name, canvas, re, im, frac = case
    raw, _ = RC.expected(case)
    cx, cy = RC.centroid(raw)
    want = (-0.5, -1.0) if name.endswith("_x") else (-1.0, -0.5)
    assert (cx, cy) == want
    assert O.psf_center_offsets(raw) == ((0, -1) if name.endswith("_x") else (-1, 0))
    assert (math.floor(cx), math.floor(cy)) == (-1, -1)


@pytest.mark.parametrize("case", [c for c in RC.exposure_cases() if c[4] <= 0], ids=lambda c: c[0])
def test_zero_and_negative_fractions_give_an_empty_psf(case):
    name, canvas, re, im, frac = case
    raw, cen = RC.expected(case)
    assert not raw.any() and not cen.any()
    assert O.psf_center_offsets(raw) == (-canvas // 2, -canvas // 2)


def test_exposure_cases_reach_both_sides_of_the_sample_cut():
    """nsamp = (int)fn + 2 is used where fn + 2 < iters: the cases stand on both sides, at 300 and at 2,000 samples."""
    sides = {300: set(), 2000: set()}
    for name, canvas, re, im, frac in RC.exposure_cases():
        sides[len(re)].add(frac * len(re) + 2.0 < len(re))
    assert sides == {300: {True, False}, 2000: {True, False}}
    fn = [f * 300 for f in RC.FRACTIONS_300]
    assert fn[0] == 0 and fn[1] < 0 and 0 < fn[2] < 1 and fn[3] == 1 and fn[4] == 2 and fn[7] == 300 and fn[8] > 300 and 299 < fn[6] < 300


def _host(case, center):
    from detectinblur_amd.motion_blur.generate_PSF import PSF
    name, canvas, re, im, frac = case
    p = PSF(canvas=canvas, trajectory=types.SimpleNamespace(x=np.asarray(re) + 1j * np.asarray(im)), fraction=[frac])
    p.fit()
    if center:
        p.centerPSF()
    return p.PSFs[0]


@pytest.mark.parametrize("case", IN_CANVAS, ids=_ids(IN_CANVAS))
def test_host_classes_match_the_oracle(case):
    raw, cen = RC.expected(case)
    assert _same(_host(case, False), raw)
    assert _same(_host(case, True), cen)


@pytest.mark.parametrize("case", IN_CANVAS, ids=_ids(IN_CANVAS))
def test_padded_restatement_matches_the_oracle(case):
    name, canvas, re, im, frac = case
    assert _same(RC.psf_rasterize_dropping(re, im, frac, canvas), RC.expected(case)[0])


@pytest.mark.parametrize("case", HIGH, ids=_ids(HIGH))
def test_high_border_raises_in_the_oracle_and_on_the_host(case):
    name, canvas, re, im, frac = case
    assert (np.floor(re) >= canvas - 1).any() or (np.floor(im) >= canvas - 1).any()
    assert (O.sample_weight(6, frac, 0, len(re)) == 0) == name.endswith("_unexposed")
    with pytest.raises(IndexError):
        O.psf_rasterize(re, im, [frac], canvas)
    with pytest.raises(IndexError, match="trajectory leaves the %d x %d canvas" % (canvas, canvas)):
        _host(case, False)
    dropped = RC.psf_rasterize_dropping(re, im, frac, canvas)
    if name.endswith("_unexposed"):
        # without weight the sample adds +0.0 only: the PSF of the trajectory with the sample moved to the centre
        re2, im2 = re.copy(), im.copy()
        re2[6] = im2[6] = canvas / 2
        assert _same(dropped, O.psf_rasterize(re2, im2, [frac], canvas)[0])


@pytest.mark.parametrize("case", HIGH, ids=_ids(HIGH))
@pytest.mark.parametrize("kind", ["numpy", "tensor"])
def test_host_resident_trajectory_outside_the_canvas_is_refused_before_the_upload(case, kind):
    """blur_ops.rasterize_psfs raises the reference's IndexError for a trajectory it receives on the host, whatever the exposure
    weight of the offending sample -- on a machine without a GPU too, because nothing has been moved to the device by then."""
    from detectinblur_amd import blur_ops
    name, canvas, re, im, frac = case
    traj = (re + 1j * im)[None]
    if kind == "tensor":
        traj = torch.from_numpy(traj)
    with pytest.raises(IndexError, match="trajectory leaves the %d x %d canvas" % (canvas, canvas)):
        blur_ops.rasterize_psfs(traj, [frac], canvas=canvas, center=False)


def test_host_check_accepts_every_in_canvas_case():
    from detectinblur_amd import blur_ops
    for name, canvas, re, im, frac in IN_CANVAS:
        blur_ops.check_trajectory_in_canvas(torch.from_numpy(re + 1j * im), canvas)
    for name, canvas, traj, fracs in BATCHES:
        blur_ops.check_trajectory_in_canvas(torch.from_numpy(traj), canvas)
    blur_ops.check_trajectory_in_canvas(torch.zeros((0, 5), dtype=torch.complex128), 64)
    # one bad sample in the last row of a batch, on the imaginary axis only
    name, canvas, traj, fracs = BATCHES[1]
    bad = traj.copy()
    bad[-1, -1] = bad[-1, -1].real + 1j * (canvas - 1)
    with pytest.raises(IndexError):
        blur_ops.check_trajectory_in_canvas(torch.from_numpy(bad), canvas)
