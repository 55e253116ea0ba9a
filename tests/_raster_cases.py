"""The PSF rasteriser's edge cases, stated once for tests/test_raster_reference.py (CPU) and tests/test_raster_edges_gpu.py.

Every function returns a list of (name, canvas, re, im, fraction): float64 coordinate arrays of one trajectory (column = real part,
row = imaginary part, as generate_PSF.py:59-61 reads them) and one exposure fraction.  Nothing is read from disk: the cases come from
seeds and small integers, and the expectation is dib_oracle's restatement of the reference (psf_rasterize, psf_center).

What each family is for (csrc/dib_raster.hip):
  random_cases       the sample loop at iters below, at and above the 256-sample ballot batch, on every canvas the entry point takes
  exposure_cases     nsamp = (int)fn + 2 against iters, and fn = fraction * iters at 0, negative, below 1, an integer, above iters
  lattice_cases      exact non-zero counts around the centroid stage's 1,024-entry staging loop, offsets of either sign
  truncation_cases   a centroid in (-1, 0): the offset truncates toward zero
  border_cases       coordinates below 1 (clamped to cell 1) and in the last legal cell
  high_border_cases  floor(coord) >= canvas - 1: the reference raises IndexError, the device drops the splats outside the canvas
  batch_cases        more than one launch chunk of 64 PSFs; every PSF has its own trajectory and its own fraction
"""
import math

import numpy as np

import dib_oracle as O
import golden_inputs as GI

CANVASES = (64, 128, 256)
MAX_LEN = {64: 20, 128: 50, 256: 96}        # the walk is max_len long in all: it stays this far from the canvas centre
RANDOM_ITERS = (2, 5, 255, 256, 257, 700)
FRACTIONS_300 = (0.0, -0.25, 1e-4, 1 / 300, 2 / 300, 0.5, 1 - 1e-12, 1.0, 1.5)
LATTICE_COUNTS = {64: (1, 1023, 1024, 1025, 2049), 128: (1025, 4097), 256: (1025, 4097)}
LOW_RE = (5, 0.25, -3.5, 1.0, 0.999, 1.5, 61.999, 62 - 1e-9)
LOW_IM = (5, 1.75, 2.5, 0.0, 1.001, -0.5, 61.5, 3.0)
BATCHES = ((64, 300, 64), (64, 300, 65), (64, 300, 130), (256, 257, 65))     # canvas, iters, B


def _walk(canvas, iters, seed, expl):
    re, im, _, _ = O.trajectory(canvas, iters, MAX_LEN[canvas], expl, np.random.RandomState(seed))
    return re, im


def random_cases():
    out = []
    for ci, canvas in enumerate(CANVASES):
        for ii, iters in enumerate(RANDOM_ITERS):
            re, im = _walk(canvas, iters, 7000 + 10 * ci + ii, GI.PARAMS[(ci + ii) % 3])
            # full exposure up to 257 samples so that the loop really runs to `iters`; 700: nsamp between two ballot batches
            frac = 1.0 if iters < 700 else 0.83
            out.append(("random_c%d_i%d" % (canvas, iters), canvas, re, im, frac))
        # iters = 1 (O.trajectory divides by iters - 1): the only sample is sample 0, whose exposure weight is zero
        h = canvas / 2
        out.append(("single_c%d" % canvas, canvas, np.array([h + 0.3]), np.array([h - 0.6]), 1.0))
    return out


def exposure_cases():
    out = []
    for ci, canvas in enumerate((64, 128)):
        re, im = _walk(canvas, 300, 7100 + ci, GI.PARAMS[ci])
        for k, f in enumerate(FRACTIONS_300):
            out.append(("exposure_c%d_i300_f%d" % (canvas, k), canvas, re, im, f))
    re, im = _walk(256, 2000, 7110, GI.PARAMS[2])
    for k in (3, 2, 1):
        out.append(("exposure_c256_i2000_m%d" % k, 256, re, im, (2000 - k) / 2000))
    return out


def lattice(canvas, n, corner):
    """Sample 0 (zero exposure weight), then n samples on distinct integer cells walked row-major over a block about sqrt(n) wide
    that starts in the canvas's first legal cell (corner "ul": centroid above and left of the centre, negative offsets) or ends in
    its last one ("lr": positive offsets).  A sample on integer coordinates gives weight to exactly one cell."""
    w = int(math.ceil(math.sqrt(n)))
    rows = -(-n // w)
    r0, c0 = (1, 1) if corner == "ul" else (canvas - 1 - rows, canvas - 1 - w)
    assert r0 >= 1 and c0 >= 1 and r0 + rows <= canvas - 1 and c0 + w <= canvas - 1
    k = np.arange(n)
    re = np.concatenate([[c0], c0 + k % w]).astype(np.float64)
    im = np.concatenate([[r0], r0 + k // w]).astype(np.float64)
    return re, im


def lattice_cases():
    out = []
    for canvas in CANVASES:
        for n in LATTICE_COUNTS[canvas]:
            for corner in ("ul", "lr"):
                re, im = lattice(canvas, n, corner)
                out.append(("lattice_c%d_n%d_%s" % (canvas, n, corner), canvas, re, im, 1.0))
    return out


def lattice_count(name):
    return int(name.split("_n")[1].split("_")[0])


def truncation_cases():
    """Samples (h, h), (h-1, h-1), (h, h-1): sample 0 has no weight, the other two put the centroid at exactly (-0.5, -1.0) from the
    centre, so the offsets are (0, -1) where a floor would give (-1, -1).  `_y` is the same with the axes exchanged: (-1, 0)."""
    out = []
    for canvas in CANVASES:
        h = canvas / 2
        a, b = np.array([h, h - 1, h]), np.array([h, h - 1, h - 1])
        out.append(("truncation_c%d_x" % canvas, canvas, a, b, 1.0))
        out.append(("truncation_c%d_y" % canvas, canvas, b, a, 1.0))
    return out


def border_cases():
    """`low`: coordinates below 1 and below 0 (clamped to cell 1, where their triangle weights mostly vanish), exactly 1.0 and 0.0,
    and two samples just under canvas - 2.  `last`: floor(coord) = canvas - 2, the last cell the reference accepts, which splats on
    row / column canvas - 1."""
    out = []
    for canvas in CANVASES:
        re, im = np.array(LOW_RE, dtype=np.float64), np.array(LOW_IM, dtype=np.float64)
        re[-2:] += canvas - 64
        im[-2] += canvas - 64
        out.append(("border_c%d_low" % canvas, canvas, re, im, 1.0))
        e = canvas - 2
        out.append(("border_c%d_last" % canvas, canvas, np.array([5, e + 0.5, 7.25, e, e + 0.999]),
                    np.array([5, 9.5, e + 0.75, e, e + 1 - 1e-9]), 1.0))
    return out


def is_low_border(name):
    return name.startswith("border_") and name.endswith("_low")


def in_canvas_cases():
    return random_cases() + exposure_cases() + lattice_cases() + truncation_cases() + border_cases()


def high_border_cases():
    """Eight samples; sample 6 leaves the canvas on the high side in x, in y, in both, or far outside.  `_full`: every sample is
    exposed.  `_unexposed`: fraction 0.5, so that the window ends at sample 4 and the offending sample has zero weight."""
    out = []
    for canvas in CANVASES:
        h, e = canvas / 2, canvas - 1
        bad = {"x": (e + 0.4, h + 0.3), "y": (h + 0.3, e + 0.6), "xy": (e + 0.25, e + 0.5), "far": (canvas + 6.5, canvas + 6.25),
               "edge": (float(e), float(e))}
        for kind, (bx, by) in bad.items():
            re = np.array([h, h + 1.3, h - 2.2, h + 0.5, h - 0.75, h + 3.125, bx, h + 1.0])
            im = np.array([h, h - 0.7, h + 0.4, h + 2.5, h - 1.25, h - 0.5, by, h + 2.0])
            out.append(("high_c%d_%s_full" % (canvas, kind), canvas, re, im, 1.0))
            out.append(("high_c%d_%s_unexposed" % (canvas, kind), canvas, re, im, 0.5))
    return out


def psf_rasterize_dropping(re, im, fraction, canvas):
    """The reference's loop (generate_PSF.py:31-83, one exposure window from 0) on a (canvas + 1)^2 accumulator, cropped to the canvas:
    "the splats on row or column `canvas` are dropped", stated without an IndexError.  Equal to O.psf_rasterize wherever that does
    not raise (tests/test_raster_reference.py)."""
    iters = len(re)
    acc = np.zeros((canvas + 1, canvas + 1), dtype=np.float64)
    for t in range(iters):
        w = O.sample_weight(t, fraction, 0, iters)
        x, y = float(re[t]), float(im[t])
        m2 = int(min(canvas - 1, max(1, math.floor(x))))
        m1 = int(min(canvas - 1, max(1, math.floor(y))))
        for (row, col) in ((m1, m2), (m1, m2 + 1), (m1 + 1, m2), (m1 + 1, m2 + 1)):
            acc[row, col] += w * (max(0.0, 1.0 - abs(x - col)) * max(0.0, 1.0 - abs(y - row)))
    return np.ascontiguousarray((acc / iters)[:canvas, :canvas])


def batch_cases():
    """[(name, canvas, trajectories [B, iters] complex128, fractions [B])]: PSF b has its own walk (seed, blur type) and its own
    fraction, so one computed from its neighbour's or its chunk-mate's trajectory or fraction differs."""
    out = []
    for k, (canvas, iters, B) in enumerate(BATCHES):
        rs = np.random.RandomState(7200 + k)
        traj = np.empty((B, iters), dtype=np.complex128)
        for b in range(B):
            re, im = _walk(canvas, iters, 7300 + 1000 * k + b, GI.PARAMS[b % 3])
            traj[b] = re + 1j * im
        fracs = [float(f) for f in rs.uniform(0.05, 1.0, B)]
        out.append(("batch_c%d_i%d_b%d" % (canvas, iters, B), canvas, traj, fracs))
    return out


def centroid(psf):
    """The centroid that psf_center_offsets truncates (same order of additions), minus canvas / 2: (x, y) as floats."""
    canvas = psf.shape[0]
    total = O.numpy_sum(psf)
    ax = ay = 0.0
    for r, c in zip(*np.nonzero(psf > 0)):
        w = float(psf[r, c]) / total
        ax += float(c) * w
        ay += float(r) * w
    return ax - canvas / 2, ay - canvas / 2


_expected = {}


def expected(case):
    """(raw, centred) float64 oracle PSFs of a single-trajectory case, computed once per process."""
    name, canvas, re, im, frac = case
    if name not in _expected:
        raw = O.psf_rasterize(re, im, [frac], canvas)[0]
        _expected[name] = (raw, O.psf_center(raw))
    return _expected[name]


def expected_batch(case):
    name, canvas, traj, fracs = case
    if name not in _expected:
        raws = [O.psf_rasterize(t.real, t.imag, [f], canvas)[0] for t, f in zip(traj, fracs)]
        _expected[name] = (np.stack(raws), np.stack([O.psf_center(r) for r in raws]))
    return _expected[name]
