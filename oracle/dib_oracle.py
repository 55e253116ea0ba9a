"""CPU oracle: a restatement of the reference's hot path in numpy.

TEST INFRASTRUCTURE -- NOT PRODUCT CODE.  Only `tests/`, `__graft_entry__.smoke()`
and `bench.py`'s `cpu_baseline` leg may import this package; the product package
`detectinblur_amd` never does (it raises if its HIP library is missing).

Every function restates, from the arithmetic spec in SURVEY.md section 8 / appendix A, one
function of mohammed-amr/detectInBlur and cites the reference file:line it follows.  It is
written in explicit real arithmetic (no complex objects, no torch.roll) so that it doubles as
the spec for the HIP kernels.

PARITY PINNING: `oracle/gen_goldens.py` imports the real reference (in the build container,
where /root/reference exists) and writes `tests/golden/*.npz`; `tests/test_oracle_golden.py`
checks this file against those vectors bit for bit (fp64 trajectories / PSFs, fp16 blur
results, fp32 boxes).  Pinned numeric environment of those runs: numpy 2.2.6, glibc 2.35,
torch 2.10 (CPU half arithmetic = fp32 compute + one rounding, which equals native fp16
arithmetic by the p_wide >= 2p+2 double-rounding theorem).

The detector (A12-A15) is NOT covered here: its arithmetic lives in an un-vendored, unpinned
torchvision -- parity unpinned for that part.
"""
import ctypes
import ctypes.util
import math

import numpy as np

# --------------------------------------------------------------------------------------
# A1  Trajectory.fit            (reference motion_blur/generate_trajectory.py:38-98)
# --------------------------------------------------------------------------------------

_libm = None


def _cexp(re, im):
    """np.exp(complex) == glibc cexp() (probe-verified; NOT equal to (cos, sin) from
    separate libm calls in ~0.16 % of arguments).  generate_trajectory.py:70."""
    z = np.exp(complex(re, im))
    return float(z.real), float(z.imag)


def _m():
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.fma.restype = ctypes.c_double
        _libm.fma.argtypes = [ctypes.c_double] * 3
        _libm.hypot.restype = ctypes.c_double
        _libm.hypot.argtypes = [ctypes.c_double] * 2
    return _libm


def _fma(a, b, c):
    return _m().fma(a, b, c)


def cabs_numpy(re, im):
    """|re + i*im| exactly as numpy >= 1.25 computes np.abs(complex128) on an FMA machine:
    max * sqrt(fma(min/max, min/max, 1)) (probe-verified 200k/200k).  generate_trajectory.py:80."""
    a, b = abs(re), abs(im)
    mx, mn = (a, b) if a >= b else (b, a)
    if mx == 0.0:
        return 0.0
    d = mn / mx
    return mx * math.sqrt(_fma(d, d, 1.0))


def trajectory(canvas=64, iters=2000, max_len=60, expl=None, rng=np.random):
    """Returns (x_re, x_im, tot_length, big_expl_count); x = x_re + i*x_im is `Trajectory.x`.

    Follows generate_trajectory.py:8-36 (constructor draw for expl=None) and :38-98 (fit).
    RNG draw order on the legacy global stream: 4x uniform, then per step uniform,
    [uniform if big shake], randn (real), randn (imag).  One call = ONE fit; the reference's
    caller runs fit twice (transforms.py:316-317)."""
    if expl is None:
        expl = 0.1 * rng.uniform(0, 1)                                    # :29
    centripetal = 0.7 * rng.uniform(0, 1)                                 # :48
    prob_big_shake = 0.2 * rng.uniform(0, 1)                              # :50
    gaussian_shake = 10 * rng.uniform(0, 1)                               # :52
    init_angle = 360 * rng.uniform(0, 1)                                  # :53
    rad = float(init_angle) * (math.pi / 180.0)                          # np.deg2rad
    v_im0 = float(np.sin(rad))                                            # :55
    v_re0 = float(np.cos(rad))                                            # :56
    step = max_len / (iters - 1)
    # :59  v = v0 * max_len / (iters-1)  (python complex: scale then true division)
    v_re = (v_re0 * max_len) / (iters - 1)
    v_im = (v_im0 * max_len) / (iters - 1)
    if expl > 0:                                                          # :61-62
        v_re = v_re0 * expl
        v_im = v_im0 * expl
    x_re = np.zeros(iters, dtype=np.float64)
    x_im = np.zeros(iters, dtype=np.float64)
    tot_length = 0.0
    big = 0
    centripetal = float(centripetal)
    gaussian_shake = float(gaussian_shake)
    threshold = float(prob_big_shake) * expl                              # :69
    for t in range(iters - 1):
        nd_re = nd_im = 0.0
        if rng.uniform() < threshold:                                     # :69
            e_re, e_im = _cexp(0.0, math.pi + (rng.uniform() - 0.5))     # :70
            a_re, a_im = 2 * v_re, 2 * v_im
            nd_re = a_re * e_re - a_im * e_im
            nd_im = a_re * e_im + a_im * e_re
            big += 1
        g_re = rng.randn()                                                # :76 (real first)
        g_im = rng.randn()
        in_re = gaussian_shake * g_re - centripetal * x_re[t]             # :75-76
        in_im = gaussian_shake * g_im - centripetal * x_im[t]
        dv_re = nd_re + (expl * in_re) * step                             # :75-77
        dv_im = nd_im + (expl * in_im) * step
        v_re = v_re + dv_re                                               # :79
        v_im = v_im + dv_im
        # :80  numpy complex128 / real == multiply by the reciprocal (Smith's form with b.imag=0)
        scl = 1.0 / cabs_numpy(v_re, v_im)
        v_re = (v_re * scl) * step
        v_im = (v_im * scl) * step
        x_re[t + 1] = x_re[t] + v_re                                      # :81
        x_im[t + 1] = x_im[t] + v_im
        # :82  builtin abs() of a complex128 scalar = glibc hypot (probe-verified), unlike np.abs above
        tot_length = tot_length + _m().hypot(x_re[t + 1] - x_re[t], x_im[t + 1] - x_im[t])
    x_re = x_re + canvas / 2                                              # :92
    x_im = x_im + canvas / 2
    return x_re, x_im, tot_length, big


# --------------------------------------------------------------------------------------
# A2  PSF.fit                    (reference motion_blur/generate_PSF.py:31-83)
# --------------------------------------------------------------------------------------

def sample_weight(t, frac, prev, iters):
    """t_proportion of sample t for exposure window (prev, frac].  generate_PSF.py:47-56."""
    fn = frac * iters
    pn = prev * iters
    if fn >= t and pn < t - 1:
        return 1
    if fn >= t - 1 and pn < t - 1:
        return fn - (t - 1)
    if fn >= t and pn < t:
        return t - pn
    if fn >= t - 1 and pn < t:
        return (frac - prev) * iters
    return 0


def psf_rasterize(x_re, x_im, fractions, canvas=256):
    """Returns the list of PSFs (cumulative over `fractions`, as the reference's shared
    accumulator makes them), each canvas x canvas float64.  generate_PSF.py:31-83.
    Row index = imaginary part, column index = real part."""
    iters = len(x_re)
    acc = np.zeros((canvas, canvas), dtype=np.float64)
    out = []
    for j, frac in enumerate(fractions):
        prev = 0 if j == 0 else fractions[j - 1]
        for t in range(iters):
            w = sample_weight(t, frac, prev, iters)
            re, im = float(x_re[t]), float(x_im[t])
            m2 = int(min(canvas - 1, max(1, math.floor(re))))             # :59
            m1 = int(min(canvas - 1, max(1, math.floor(im))))             # :61
            for (row, col) in ((m1, m2), (m1, m2 + 1), (m1 + 1, m2), (m1 + 1, m2 + 1)):  # :64-75
                tri = max(0.0, 1.0 - abs(re - col)) * max(0.0, 1.0 - abs(im - row))
                acc[row, col] += w * tri
        out.append(acc / iters)                                           # :77
    return out


# --------------------------------------------------------------------------------------
# A3  PSF.centerPSF              (reference motion_blur/generate_PSF.py:106-123)
# --------------------------------------------------------------------------------------

def _pairwise(a):
    """numpy's DOUBLE pairwise_sum: blocks of <=128 with 8 interleaved accumulators combined as
    ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)); larger inputs split at n/2 rounded down to x8."""
    n = a.size
    if n < 8:
        s = 0.0
        for v in a:
            s += float(v)
        return s
    if n <= 128:
        r = [float(a[i]) for i in range(8)]
        i = 8
        while i < n - (n % 8):
            for k in range(8):
                r[k] += float(a[i + k])
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < n:
            res += float(a[i])
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return _pairwise(a[:n2]) + _pairwise(a[n2:])


def numpy_sum(a):
    """np.sum of a contiguous float64 array restated (probe-verified bit for bit on 1-D and
    2-D inputs, numpy 2.2.6): the flattened data is consumed in iterator chunks of 8192
    elements; each chunk is pairwise-summed and the chunk sums are accumulated left to right."""
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    s = 0.0
    for i in range(0, a.size, 8192):
        s += _pairwise(a[i:i + 8192])
    return s


def psf_center_offsets(psf):
    """(offsetX, offsetY) of generate_PSF.py:106-120: weighted centroid of psf>0 cells,
    accumulated in np.nonzero (row-major) order, minus canvas/2, truncated toward zero."""
    canvas = psf.shape[0]
    total = numpy_sum(psf)                                             # :108  np.sum
    rows, cols = np.nonzero(psf > 0)                                      # :110
    ax = 0.0
    ay = 0.0
    for r, c in zip(rows, cols):                                          # :113-117
        w = float(psf[r, c]) / total
        ax += float(c) * w
        ay += float(r) * w
    return int(ax - canvas / 2), int(ay - canvas / 2)                     # :119-120


def psf_center(psf):
    """generate_PSF.py:106-123: roll the centroid to the canvas centre (circular)."""
    ox, oy = psf_center_offsets(psf)
    n = psf.shape[0]
    ri = (np.arange(n) + oy) % n
    ci = (np.arange(n) + ox) % n
    return psf[np.ix_(ri, ci)].copy()


def psf_crop128(psf):
    """transforms.py:334-335 / :308-309: centre 128x128 window of a 256 canvas."""
    if psf.shape[0] > 128:
        return psf[64:192, 64:192]
    return psf


def make_psf(param, fraction, canvas=256, max_len=96, rng=np.random, center=True):
    """On-the-fly PSF exactly as BlurImage builds it (transforms.py:316-335): two trajectory
    fits (the first only advances the RNG), rasterise, centre, crop."""
    trajectory(canvas, 2000, max_len, param, rng)
    x_re, x_im, _, _ = trajectory(canvas, 2000, max_len, param, rng)
    psf = psf_rasterize(x_re, x_im, [fraction], canvas)[0]
    if not center:
        return psf
    return np.ascontiguousarray(psf_crop128(psf_center(psf)))


# --------------------------------------------------------------------------------------
# A6  host -> device PSF conversion         (reference engine.py:84)
# --------------------------------------------------------------------------------------

def to_half_like_torch(a):
    """torch.HalfTensor(ndarray): float64 -> float32 -> float16 (two roundings; probe-verified
    on 2e6 values, differs from a direct float64->float16 cast in ~5e-5 of them)."""
    a = np.asarray(a)
    if a.dtype == np.float16:
        return a.copy()
    return a.astype(np.float32).astype(np.float16)


# --------------------------------------------------------------------------------------
# A7/A8  blur_image_list / manual_blur       (reference models/blur_functions.py:11-100)
# --------------------------------------------------------------------------------------

def half_sum_exact(psf_h):
    """psf.sum() of a Half tensor, defined here as the exactly-rounded sum: every finite fp16
    is a multiple of 2^-24, so the sum is exact in integers and rounded once to fp16
    (blur_functions.py:98).  torch accumulates in fp32 in an implementation-defined order and
    rounds to fp16; the two agree unless the fp32 error straddles an fp16 rounding boundary
    (never observed on the golden PSFs)."""
    q = np.asarray(psf_h, dtype=np.float16).astype(np.float64) * float(1 << 24)
    total = int(np.sum(q.astype(np.int64)))
    return np.float16(total / float(1 << 24)) if abs(total) < (1 << 53) else _round_int_to_half(total)


def _round_int_to_half(total):
    # exact integer (units of 2^-24) -> fp16 round-to-nearest-even without going through fp64
    sign = -1 if total < 0 else 1
    m = abs(total)
    if m == 0:
        return np.float16(0)
    nbits = m.bit_length()
    if nbits <= 11:
        return np.float16(sign * m * 2.0 ** -24)
    shift = nbits - 11
    q, rem = m >> shift, m & ((1 << shift) - 1)
    half = 1 << (shift - 1)
    if rem > half or (rem == half and (q & 1)):
        q += 1
    return np.float16(sign * float(q) * 2.0 ** (shift - 24))


def normalize_psf(psf):
    """psf / psf.sum() in the PSF's own dtype (blur_functions.py:98, utils.py:372)."""
    psf = np.asarray(psf)
    if psf.dtype == np.float16:
        return (psf / half_sum_exact(psf)).astype(np.float16)
    return (psf / psf.sum(dtype=psf.dtype)).astype(psf.dtype)


def taps_of(psf_norm):
    """Row-major non-zero list of a normalised PSF: (rows, cols, weights).
    blur_functions.py:63 (`nonzero(as_tuple=False)` order = ascending row, then column)."""
    rows, cols = np.nonzero(psf_norm)
    return rows.astype(np.int64), cols.astype(np.int64), psf_norm[rows, cols]


def _pad_index(s, n, mode):
    """Maps an un-padded coordinate s (may lie outside [0,n)) to a source index, or -1 = zero.
    'reflect' has no edge repeat (appendix A.1); 'replicate' clamps; 'constant' zero-fills."""
    s = np.asarray(s)
    if mode == "reflect":
        s = np.where(s < 0, -s, s)
        s = np.where(s > n - 1, 2 * (n - 1) - s, s)
        return s
    if mode == "replicate":
        return np.clip(s, 0, n - 1)
    return np.where((s < 0) | (s > n - 1), -1, s)


SEG_ROWS, SEG_COLS = 12, 24      # a tap segment's bounding box: at most 13 PSF rows x 25 columns (include/dib.h, `Tap tables`)


def tap_segments(rows, cols, seg_rows=SEG_ROWS, seg_cols=SEG_COLS):
    """The library's cut of the row-major tap list into the segments its blur stages in LDS (include/dib.h): greedy runs of
    consecutive taps whose rows span at most seg_rows + 1 and whose columns span at most seg_cols + 1.  Returns [(first, end)].
    Not the reference's arithmetic -- the reference has no segments -- but what fixes the ORDER in which DIB_ACC_FAST16 adds."""
    out, start = [], 0
    n = len(rows)
    while start < n:
        r0, cmin, cmax, end = rows[start], cols[start], cols[start], start
        while end < n:
            lo, hi = min(cmin, cols[end]), max(cmax, cols[end])
            if rows[end] - r0 > seg_rows or hi - lo > seg_cols:
                break
            cmin, cmax, end = lo, hi, end + 1
        out.append((start, end))
        start = end
    return out


def tap_order_vruns(rows, cols):
    """The order in which DIB_ACC_FAST16 (include/dib.h) accumulates the taps: segment by segment; inside a segment the taps of one
    PSF column in consecutive rows form a vertical run; a run of L taps is cut, from its lowest row up, into L // 4 groups of four
    and one group of L % 4; the segment's groups are taken by size -- all fours, then the threes, the twos, the singles -- inside a
    size in the row-major order of the runs' first taps (a run's fours from its lowest rows up), a group from its lowest row to its
    highest.  Returns a permutation of range(len(rows))."""
    order = []
    for a, b in tap_segments(rows, cols):
        index = {(int(rows[j]), int(cols[j])): j for j in range(a, b)}
        by_size = {4: [], 3: [], 2: [], 1: []}
        for j in range(a, b):
            r, c = int(rows[j]), int(cols[j])
            if (r - 1, c) in index:
                continue
            run = []
            while (r, c) in index:
                run.append(index[(r, c)])
                r += 1
            for k in range(0, len(run) - len(run) % 4, 4):
                by_size[4].append(run[k:k + 4])
            if len(run) % 4:
                by_size[len(run) % 4].append(run[len(run) - len(run) % 4:])
        for n in (4, 3, 2, 1):
            for g in by_size[n]:
                order.extend(g)
    assert sorted(order) == list(range(len(rows)))
    return order


def manual_blur(image, psf_norm, fp32_accumulate=False, fma16=False, tap_order=None):
    """models/blur_functions.py:11-69 (both canvas branches), post-ops excluded.

    fp32_accumulate=True restates the library's DIB_ACC_FP32 mode instead of the reference
    arithmetic (fp16 images only): the fp16 x fp16 products are exact in float32, the running sum is
    float32, taps in the same order, one rounding to fp16 at the end.
    fma16=True restates DIB_ACC_FMA16: acc = fp16(acc + P * w) with ONE rounding per tap (a fused
    multiply-add in fp16).  float64 holds acc + P * w exactly whenever the rounding could go either way
    (22-bit product, 11-bit accumulator), so rounding the float64 sum to fp16 is the fused result.
    tap_order: a permutation of the row-major tap list, the order to accumulate in (fma16=True with
    tap_order=tap_order_vruns(rows, cols) restates DIB_ACC_FAST16).

    image: C x H x W float16 or float32;  psf_norm: K x K, same dtype, already normalised.
    out[ch,y,x] = sum over taps (r,c), row-major, of  rnd(rnd(P[(y+2pb-r) mod Hp, (x+2pb-c) mod Wp] * w) + acc)
    with pb = K/2-1, pa = K/2, Hp = H+K-1 and P the padded image (appendix A.2/A.3)."""
    image = np.asarray(image)
    dt = image.dtype
    squeeze_c = False
    if image.ndim == 2:
        image = image[None]
        squeeze_c = True
    C, H, W = image.shape
    K = psf_norm.shape[0]
    if K > 129:                                                           # :17
        big, mode = 256, "replicate"                                      # :24-31
    else:
        big = 128
        mode = "constant" if (H < 64 or W < 64) else "reflect"            # :55-58
    pb, pa = big // 2 - 1, big // 2                                       # :52 / :26
    if mode == "reflect" and (H <= pa or W <= pa):
        raise RuntimeError("Padding size should be less than the corresponding input dimension")
    Hp, Wp = H + pb + pa, W + pb + pa
    src_r = _pad_index(np.arange(Hp) - pb, H, mode)
    src_c = _pad_index(np.arange(Wp) - pb, W, mode)
    rows, cols, wts = taps_of(np.asarray(psf_norm).astype(dt))
    acc = np.zeros((C, H, W), dtype=np.float32 if fp32_accumulate else dt)   # :61
    ys, xs = np.arange(H), np.arange(W)
    if tap_order is not None:
        rows, cols, wts = rows[list(tap_order)], cols[list(tap_order)], wts[list(tap_order)]
    for r, c, w in zip(rows, cols, wts):                                  # :66-67
        pr = src_r[(ys + 2 * pb - r) % Hp]
        pc = src_c[(xs + 2 * pb - c) % Wp]
        g = image[:, np.maximum(pr, 0)][:, :, np.maximum(pc, 0)]
        if mode == "constant":
            g = g * ((pr >= 0)[None, :, None] & (pc >= 0)[None, None, :]).astype(dt)
        if fma16:
            acc = (acc.astype(np.float64) + g.astype(np.float64) * np.float64(w)).astype(dt)
        elif fp32_accumulate:
            acc = acc + g.astype(np.float32) * np.float32(w)
        else:
            acc = (acc + (g * dt.type(w)).astype(dt)).astype(dt)
    out = acc.astype(dt)
    # :69 `.squeeze()` drops every size-1 dim
    return np.squeeze(out)


def blur_image_list(images, blur_dicts, psfs):
    """models/blur_functions.py:92-100: in-place replacement of the blurred entries."""
    for i, (img, bd, psf) in enumerate(zip(images, blur_dicts, psfs)):
        if not bd["blurring"]:
            continue
        images[i] = manual_blur(img, normalize_psf(psf))


# --------------------------------------------------------------------------------------
# A9/A10  expand_targets / fix_bounding_box_squeeze   (reference utils.py:360-434)
# --------------------------------------------------------------------------------------

def psf_extents(psf):
    """(left, top, right, bottom) = (min col, min row, max col, max row) - 63 over the
    non-zeros of the normalised PSF.  utils.py:372-380."""
    if psf.shape[0] != 128:
        raise Exception("Trying to expand with filters that are not 128 wide!")   # :369-370
    rows, cols, _ = taps_of(normalize_psf(psf))
    return int(cols.min()) - 63, int(rows.min()) - 63, int(cols.max()) - 63, int(rows.max()) - 63


def clamp_boxes(boxes, H, W):
    """utils.py:395-434 on an N x 4 float32 xyxy array (returns a new array)."""
    b = np.array(boxes, dtype=np.float32, copy=True)

    def clamp():
        b[:, 0] = np.where(b[:, 0] > W - 1, np.float32(W - 1), b[:, 0])   # :398
        b[:, 1] = np.where(b[:, 1] > H - 1, np.float32(H - 1), b[:, 1])   # :399
        b[:, 2] = np.where(b[:, 2] > W - 1, np.float32(W - 1), b[:, 2])   # :401
        b[:, 3] = np.where(b[:, 3] > H - 1, np.float32(H - 1), b[:, 3])   # :402
        b[...] = np.where(b < 0, np.float32(0), b)                        # :405-409

    clamp()
    bad = b[:, 0] >= b[:, 2]                                              # :412-414
    b[bad, 2] += np.float32(1)
    b[bad, 0] -= np.float32(1)
    bad = b[:, 1] >= b[:, 3]                                              # :416-418
    b[bad, 3] += np.float32(1)
    b[bad, 1] -= np.float32(1)
    clamp()                                                               # :421-432
    return b


def expand_boxes(boxes, psf, H, W):
    """utils.py:360-392 for one image: grow by the PSF extents, then clamp."""
    left, top, right, bottom = psf_extents(psf)
    b = np.array(boxes, dtype=np.float32, copy=True)
    b[:, 0] = b[:, 0] + np.float32(left)                                  # :382
    b[:, 2] = b[:, 2] + np.float32(right)                                 # :383
    b[:, 1] = b[:, 1] + np.float32(top)                                   # :385
    b[:, 3] = b[:, 3] + np.float32(bottom)                                # :386
    return clamp_boxes(b, H, W)


# --------------------------------------------------------------------------------------
# A4(vii)  PSF principal-axis statistics      (reference transforms.py:366-385)
# --------------------------------------------------------------------------------------

def psf_axis_stats(psf):
    """Returns (theta_rad, scale_factor_lambda1, scale_factor_lambda2)."""
    ys, xs = np.nonzero(psf > 0)
    yp = ys - ys.mean()
    xp = xs - xs.mean()
    cov = (yp * xp).mean()
    var_x = (xp * xp).mean()
    var_y = (yp * yp).mean()
    root = math.sqrt(math.pow((var_x - var_y) / 2, 2) + math.pow(cov, 2))
    lam1 = (var_x + var_y) / 2 + root
    lam2 = (var_x + var_y) / 2 - root

    def sig(v):
        return 1 / (1 + math.exp(-v))

    s1 = 1 - (sig(math.sqrt(lam1) / 10) - 0.5) * 0.6
    s2 = 1 - (sig(math.sqrt(lam2) / 10) - 0.5) * 0.6
    theta = -math.atan2(lam1 - var_x, -cov)
    return theta, s1, s2


# --------------------------------------------------------------------------------------
# A11  get_norm_params                        (reference utils.py:219-273)
# --------------------------------------------------------------------------------------

_CANON_MEAN = [0.485, 0.456, 0.406]
_CANON_STD = [0.229, 0.224, 0.225]
# per-exposure std tables (columns: clean, E0..E4), utils.py:228-230
_STD = {
    0: [[0.2384, 0.2334, 0.2370], [0.2337, 0.2288, 0.2325], [0.2270, 0.2221, 0.2261],
        [0.2209, 0.2161, 0.2203], [0.2127, 0.2082, 0.2126], [0.2087, 0.2043, 0.2088]],
    1: [[0.2384, 0.2334, 0.2370], [0.2337, 0.2287, 0.2325], [0.2267, 0.2218, 0.2258],
        [0.2184, 0.2137, 0.2180], [0.2048, 0.2006, 0.2051], [0.1950, 0.1911, 0.1957]],
    2: [[0.2384, 0.2334, 0.2370], [0.2337, 0.2287, 0.2325], [0.2266, 0.2217, 0.2258],
        [0.2182, 0.2136, 0.2178], [0.2012, 0.1972, 0.2017], [0.1824, 0.1790, 0.1838]],
}


def norm_params(blur_dicts, use_custom_image_norm):
    if blur_dicts is None:
        return np.array([_CANON_MEAN]), np.array([_CANON_STD])
    means = np.zeros((len(blur_dicts), 3))
    stds = np.zeros((len(blur_dicts), 3))
    for i, bd in enumerate(blur_dicts):
        if use_custom_image_norm and bd["blurring"] and bd["param_index"] is not None:   # :254
            fi = bd["fraction_index"]
            pi = bd["param_index"]
            if fi == -1:                                                  # :258-261
                means[i], stds[i] = _CANON_MEAN, _CANON_STD
            elif pi in (0, 1, 2):                                         # :263-271
                means[i] = _CANON_MEAN
                stds[i] = ((np.asarray(_STD[pi]).T * 0.229) / 0.2384)[:, fi + 1]
            # any other param_index (e.g. -1 from the stored-PSF off-by-one, transforms.py:427-428)
            # leaves the row at its initial zeros, as the reference does
        else:
            means[i], stds[i] = _CANON_MEAN, _CANON_STD
    return means, stds


# --------------------------------------------------------------------------------------
# A18  BlurImageHandler (--cpu_blur, FFT)     (reference motion_blur/blur_image.py:23-154)
# --------------------------------------------------------------------------------------

def _minmax01(a):
    """cv2.normalize(..., 0, 1, NORM_MINMAX, CV_32F): global min/max over all channels."""
    a = np.asarray(a, dtype=np.float64)
    lo, hi = float(a.min()), float(a.max())
    scale = 1.0 / (hi - lo) if hi > lo else 0.0
    return ((a - lo) * scale).astype(np.float32)


def cpu_fft_blur(image_u8, psf):
    """`--cpu_blur`: image_u8 H x W x 3 uint8, psf k x k (k <= H, W) -> H x W x 3 uint8.
    blur_image.py:78-85 (edge pad k/2), :113-123 (zero-pad the PSF to the image), :128-134
    (min-max, fftconvolve 'same' per channel, min-max), :137-147 (un-pad, x255 -> uint8).
    The upscale branch for images smaller than the PSF (:56-69) is not restated (bicubic PIL
    resize + cv2 Lanczos); such inputs raise."""
    from scipy import signal
    img = np.asarray(image_u8)
    H, W = img.shape[:2]
    k = psf.shape[0]
    if H < k or W < k:
        raise NotImplementedError("image smaller than the PSF: resize branch not restated")
    pr = int(round(k / 2))
    orig = np.pad(img, ((pr, pr), (pr, pr), (0, 0)), mode="edge")
    yN, xN = orig.shape[:2]
    dY, dX = yN - k, xN - k
    tmp = np.pad(np.asarray(psf, dtype=np.float32),
                 ((dY // 2, math.ceil(dY / 2)), (math.ceil(dX / 2), dX // 2)), "constant")
    tmp = _minmax01(tmp)
    blurred = _minmax01(orig)
    for ch in range(3):
        blurred[:, :, ch] = signal.fftconvolve(blurred[:, :, ch], tmp, "same")
    blurred = _minmax01(blurred)
    blurred = blurred[pr:blurred.shape[0] - pr, pr:blurred.shape[1] - pr, :]
    return (blurred * 255).astype(np.uint8)


# --------------------------------------------------------------------------------------
# A16 post-blur corruption chain: noise + clamp, block artefacts, JPEG round trip
#     (reference models/blur_functions.py:72-87, transforms.py:467-493, models/jpeg/*)
# --------------------------------------------------------------------------------------
# Float64 references for the two post-op kernels (csrc/dib_postops.hip, csrc/dib_jpeg.hip).  Each returns the expected
# result together with what float64 cannot decide about the kernel's fp32 arithmetic: a per-pixel error bound (JPEG) or
# the set of elements whose fp16 rounding is not determined (noise).

_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counters, key):
    """Philox-4x32-10 (Salmon et al., SC'11; the Random123 definition) on an array of counters [..., 4] (uint32) under
    the key (k0, k1): ten rounds, the key bumped by the Weyl constants after each.  dib_postops.hip philox_round."""
    c = np.asarray(counters, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i] & _U32 for i in range(4))
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = c0 * np.uint64(0xD2511F53)          # < 2^64: exact in uint64
        p1 = c2 * np.uint64(0xCD9E8D57)
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _U32
        k0 = (k0 + np.uint64(0x9E3779B9)) & _U32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _U32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def post_ops_key(torch_seed):
    """The noise field's key as blur_ops.post_ops draws it: one int64 from torch's host generator after
    torch.manual_seed(torch_seed).  Returns (key0, key1) = (low, high) 32-bit words."""
    import torch
    torch.manual_seed(torch_seed)
    s = int(torch.empty((), dtype=torch.int64).random_().item()) & 0xFFFFFFFFFFFFFFFF
    return s & 0xFFFFFFFF, s >> 32


def normal64(index, key):
    """The kernel's normal at each element index (dib_postops.hip normal_at): Philox on counter (index, 0, 0, 0), the two
    uniforms formed in float32 exactly as the kernel forms them (`(float)(w >> 8) + 0.5f` rounds above 2^23), the angle
    2 pi u2 rounded to float32 as the kernel's product is; then Box-Muller in float64.  The kernel's __logf / __cosf /
    sqrtf and its two fp32 products differ from this by at most eps_n (measured: tests/test_postops_reference.py)."""
    index = np.asarray(index, dtype=np.uint64)
    ctr = np.zeros(index.shape + (4,), dtype=np.uint64)
    ctr[..., 0] = index & _U32
    ctr[..., 1] = index >> np.uint64(32)
    w = philox4x32_10(ctr, key)
    inv = np.float32(1.0 / 16777216.0)
    u1 = ((w[..., 0] >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * inv
    u2 = ((w[..., 1] >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * inv
    ang = np.float32(6.28318530717958647692) * u2
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(ang.astype(np.float64))


def _half_boundary_distance(n):
    """Distance of each float64 `n` from the nearest fp16 round-to-nearest boundary (midpoint of two adjacent halves)."""
    h = n.astype(np.float16)
    up = np.nextafter(h, np.float16(np.inf)).astype(np.float64)
    dn = np.nextafter(h, np.float16(-np.inf)).astype(np.float64)
    hd = h.astype(np.float64)
    return np.minimum(np.abs(n - (hd + up) / 2), np.abs(n - (hd + dn) / 2))


def block_source_map(H, W, block_scale):
    """Source row / column of every output row / column under the block arm: interpolate(scale_factor=s) then
    interpolate(size=(H, W)), both 'nearest' (blur_functions.py:76-81), composed as dib_postops.hip does it in fp32 --
    ATen upsample_nearest2d's src = min(floor(dst * scale), in - 1) with scale = float(1 / s) for the first call and
    float(in) / out for the second; the first call's size = floor(double(in) * s)."""
    if not block_scale:
        return np.arange(H), np.arange(W)
    f32 = np.float32
    hs, ws = int(math.floor(H * block_scale)), int(math.floor(W * block_scale))
    down = f32(1.0 / block_scale)
    up_h, up_w = f32(hs) / f32(H), f32(ws) / f32(W)

    def comp(n, m, up):
        mid = np.minimum(np.floor(np.arange(n, dtype=np.float32) * up).astype(np.int64), m - 1)
        return np.minimum(np.floor(mid.astype(np.float32) * down).astype(np.int64), n - 1)
    return comp(H, hs, up_h), comp(W, ws, up_w)


def post_ops64(img, noise_var, block_scale, seed, eps_n):
    """Expected output of dib_post_ops on a C x H x W (or H x W) float16 / float32 image (blur_functions.py:72-81 as
    the kernel computes it), and the mask of output elements whose value is not determined by float64.

    seed: the torch.manual_seed value in force when blur_ops.post_ops draws the key (post_ops_key).
    Noise: element (c, y, x) reads source (c, sy, sx) through the composed block maps and adds the normal at counter
    c*H*W + sy*W + sx.  float16: n16 = half(n), prod = half(float(n16) * float(std)), out = half(v + prod), clamp --
    each step restated exactly in numpy's IEEE float32 / float16; only n comes from the kernel's approximate __logf /
    __cosf, so an element is not determined when n lies within eps_n of an fp16 rounding boundary AND the two
    candidate n16 on either side give different outputs (given n16, the rest -- clamp included, which acts on an fp16
    value -- is exact).  float32: out = v + f32(n * std), clamp; the
    expected value uses float64 n and the mask is empty -- compare within eps_n * std plus one ulp."""
    a = np.asarray(img)
    if a.dtype not in (np.float16, np.float32):
        raise TypeError("post_ops64: float16 / float32 image")
    x = a[None] if a.ndim == 2 else a
    C, H, W = x.shape
    undet = np.zeros(x.shape, dtype=bool)
    out = x.copy()
    if noise_var:
        std = np.float32(math.sqrt(noise_var))
        key = post_ops_key(seed)
        n = normal64(np.arange(C * H * W, dtype=np.uint64), key).reshape(C, H, W)
        if x.dtype == np.float16:
            def half_chain(n16):
                prod = (n16.astype(np.float32) * std).astype(np.float16)
                o = (x.astype(np.float32) + prod.astype(np.float32)).astype(np.float16)
                return np.minimum(np.maximum(o, np.float16(0)), np.float16(1))
            out = half_chain(n.astype(np.float16))
            # the kernel's n lies in [n - eps_n, n + eps_n]: eps_n << one fp16 ulp, so at most one rounding boundary is
            # in reach and half(n - eps_n), half(n + eps_n) are the only candidates for its n16
            near = _half_boundary_distance(n) <= eps_n
            undet = near & (half_chain((n - eps_n).astype(np.float16)).view(np.uint16) != half_chain((n + eps_n).astype(np.float16)).view(np.uint16))
        else:
            out = x + (n.astype(np.float32) * std)
            out = np.minimum(np.maximum(out, np.float32(0)), np.float32(1))
    sy, sx = block_source_map(H, W, block_scale)
    out, undet = out[:, sy][:, :, sx], undet[:, sy][:, :, sx]
    if a.ndim == 2:
        out, undet = out[0], undet[0]
    return out, undet


# JPEG round trip ------------------------------------------------------------------------
# Standard tables as the reference holds them: models/jpeg/utils.py:7-21 (transposed: indexed [u][v]).
JPEG_LUMA = np.array([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56],
                      [14, 17, 22, 29, 51, 87, 80, 62], [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92],
                      [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]], dtype=np.float32).T
JPEG_CHROMA = np.full((8, 8), 99, dtype=np.float32)
JPEG_CHROMA[:4, :4] = np.array([[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]], dtype=np.float32).T


def jpeg_quality_factor(quality):
    """models/jpeg/utils.py:34-45."""
    q = 5000.0 / quality if quality < 50 else 200.0 - quality * 2
    return q / 100.0 if quality < 50 else (q + 0.01) / 100.0


# The colour matrices are the reference's fp32 buffers (compression.py:20-22, decompression.py:102-115): every
# implementation multiplies by these fp32 values, so the float64 chain starts from them, exactly.
_f64 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float64)   # noqa: E731
_TO_YCC = _f64([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]])
_TO_RGB = _f64([[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]])
_COS8 = np.cos((2 * np.arange(8)[:, None] + 1) * np.arange(8)[None, :] * np.pi / 16)     # [a, u]
_ALPHA = np.array([1 / np.sqrt(2)] + [1.0] * 7)
_AA4 = np.outer(_ALPHA, _ALPHA) / 4
_U = 2.0 ** -24                                                   # fp32 unit roundoff


def _gamma(n):
    return n * _U / (1 - n * _U)


def _blocks(p):        # [h, w] -> [h/8, w/8, 8, 8]
    return p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).transpose(0, 2, 1, 3)


def _planes(b):
    return b.transpose(0, 2, 1, 3).reshape(b.shape[0] * 8, b.shape[1] * 8)


def _code_decode(plane, q):
    """One plane (pixel values - 128) through DCT, quantise, dequantise, inverse DCT.  Returns the decoded plane (+128),
    the per-pixel bound of one quantisation step of every ambiguous coefficient of its block, the per-pixel fp32 error
    of the inverse transform, and the per-block ambiguity flag.

    Ambiguity threshold delta (per block, per coefficient), from the fp32 arithmetic of every implementation:
      inputs: each Y / Cb / Cr value is x*255 and a 3-term dot with |row| <= 1 plus a shift (<= 383 in magnitude), the
        chroma 2x2 mean and the -128 add two more steps: <= 10 roundings of values <= 383, e_in = 10 u 383;
      the coefficient c = alpha_u alpha_v / 4 sum_ab blk cos cos: 64 products summed in ANY order (the kernel's nested
        8 x 8, a GEMM's blocked order, the CPU tensordot) err <= gamma_64 S with S = sum |blk|; the basis (cosf or the
        fp32 table) and the products before the sum add <= 10 u S; the input error adds <= 64 e_in (|cos cos| <= 1);
        the alpha / 4 scale and the division by q one rounding each of |c| and |c / q|.
      delta_uv = alpha_u alpha_v / 4 (gamma_64 S + 10 u S + 64 e_in) / q_uv + 3 u |c / q_uv|.
    A coefficient with |frac(c / q) - 0.5| < delta may round either way and is ambiguous: one step q_uv either way,
    which the inverse transform carries to pixel (a, b) as alpha_u alpha_v / 4 q_uv |cos_au cos_bv|.
    With no ambiguous coefficient the integers are the same, and the decoded pixel differs by the fp32 error of the
    inverse transform alone: a 64-term sum of |alpha deq cos cos| / 4 (T), any order, plus 10 u T for the basis and
    the dequantising products, and the +128."""
    b = _blocks(plane)
    c = _AA4 * np.einsum("au,hwab,bv->hwuv", _COS8, b, _COS8)
    ratio = c / q
    S = np.abs(b).sum(axis=(2, 3))[..., None, None]
    e_in = 10 * _U * 383.0
    delta = _AA4 * ((_gamma(64) + 10 * _U) * S + 64 * e_in) / q + 3 * _U * np.abs(ratio)
    amb = np.abs(ratio - np.floor(ratio) - 0.5) < delta
    deq = np.rint(ratio) * q
    dec = np.einsum("au,hwuv,bv->hwab", _COS8, _AA4 * deq, _COS8) + 128
    flip = np.einsum("au,hwuv,bv->hwab", np.abs(_COS8), np.where(amb, _AA4 * q, 0.0), np.abs(_COS8))
    T = (np.abs(_AA4 * deq)).sum(axis=(2, 3))[..., None, None]
    err = ((_gamma(64) + 10 * _U) * T + 2 * _U * 1152.0) * np.ones_like(dec)
    return _planes(dec), _planes(flip), _planes(err), amb.any(axis=(2, 3))


def jpeg_roundtrip64(img, quality, pad=True):
    """transforms.add_jpeg_artifact_to_image (transforms.py:467-493) around DiffJPEG (models/jpeg/DiffJPEG.py:
    compression.py + decompression.py, rounding = torch.round) in float64 from the input's exact values, on one
    3 x H x W image in [0, 1].  Returns (expected, bound, exact):
      expected  3 x H x W float64 -- the round trip's value before the final fp16 cast;
      bound     3 x H x W float64 -- |fp16 result - expected| allowed at each pixel: 1/2 fp16 ulp + the fp32 error of the
                chain with the same quantised integers, + one quantisation step carried through the inverse DCT and the
                colour matrix for every ambiguous coefficient of the blocks the pixel reads (see _code_decode);
      exact     H x W bool -- the pixel's luma block and chroma blocks have no ambiguous coefficient.
    pad=False: DiffJPEG alone on an image whose sides are multiples of 16 (no reflect pad / crop)."""
    x = np.asarray(img).astype(np.float64)
    _, H, W = x.shape
    wp, hp = (16 - W % 16, 16 - H % 16) if pad else (0, 0)     # transforms.py:471-477: a full 16 when already a multiple
    left, top = wp // 2, hp // 2
    xp = np.pad(x, ((0, 0), (top, hp - top), (left, wp - left)), mode="reflect")
    ycc = np.einsum("ij,jhw->ihw", _TO_YCC, xp * 255) + np.array([0.0, 128.0, 128.0])[:, None, None]
    Hp, Wp = ycc.shape[1:]
    pooled = ycc[1:].reshape(2, Hp // 2, 2, Wp // 2, 2).mean(axis=(2, 4))                  # avg_pool2d(2, 2)
    fac = np.float32(jpeg_quality_factor(quality))
    qy = (JPEG_LUMA * fac).astype(np.float64)
    qc = (JPEG_CHROMA * fac).astype(np.float64)
    y, fy, ey, ay = _code_decode(ycc[0] - 128, qy)
    chans, flips, errs, ambs = [y], [fy], [ey], [np.kron(ay, np.ones((8, 8), dtype=bool))]
    for k in (0, 1):
        d, f, e, a = _code_decode(pooled[k] - 128, qc)
        up = lambda p: p.repeat(2, axis=0).repeat(2, axis=1)      # noqa: E731
        chans.append(up(d)); flips.append(up(f)); errs.append(up(e))
        ambs.append(np.kron(a, np.ones((16, 16), dtype=bool)))
    ycc_dec = np.stack(chans) - np.array([0.0, 128.0, 128.0])[:, None, None]
    rgb = np.einsum("ij,jhw->ihw", _TO_RGB, ycc_dec)
    A = np.abs(_TO_RGB)
    flip = np.einsum("ij,jhw->ihw", A, np.stack(flips))
    # the decoded planes' fp32 errors through the colour matrix, + 4 roundings of values <= 1152 (-128, products, sums),
    # the clamp is 1-Lipschitz, / 255 one more rounding
    err = np.einsum("ij,jhw->ihw", A, np.stack(errs)) + 4 * _U * 1152.0
    out = np.clip(rgb, 0, 255) / 255
    crop = (slice(None), slice(top, top + H), slice(left, left + W))
    out, flip, err = out[crop], flip[crop] / 255, err[crop] / 255 + _U
    exact = ~(ambs[0] | ambs[1] | ambs[2])[top:top + H, left:left + W]
    hi = np.abs(out) + flip + err
    half_ulp = np.spacing(hi.astype(np.float16)).astype(np.float64) / 2       # the final cast to fp16
    return out, flip + err + half_ulp, exact


# --------------------------------------------------------------------------------------
# A17 RoIAlign and greedy NMS: float64 / exact-integer references for csrc/dib_roi.hip
#     (torchvision.ops.roi_align / nms, which reference models/faster_rcnn.py:204-208 and its RPN / RoIHeads call)
# --------------------------------------------------------------------------------------
# Written from the published Detectron / torchvision definition, not from the kernels.  Per RoI (batch index, x1, y1,
# x2, y2) on an H x W map: corners times spatial_scale (minus 0.5 when aligned); width / height clamped to >= 1 unless
# aligned; P x P bins; per bin a gh x gw grid of samples at bin start + (i + 0.5) * bin / g, g = sampling_ratio or,
# when that is <= 0, ceil(size / P) per axis; a sample with y < -1, y > H, x < -1 or x > W counts 0, every other one is
# the bilinear interpolation at (max(y, 0), max(x, 0)) with the last row / column repeated beyond H - 1 / W - 1; the bin
# is the sum over max(gh * gw, 1).  All arithmetic in float64 from the float32 inputs.

def _roi_axis(lo, bin_, P, g, L, guard, force):
    """Sample coordinates of one axis for K RoIs with a common grid g: [K, P * g] -> inside, near, i0, i1, w0, w1."""
    frac = (np.arange(P)[:, None] + (np.arange(g)[None, :] + 0.5) / g).reshape(-1)
    t = lo[:, None] + frac[None, :] * bin_[:, None]
    near = (np.abs(t + 1.0) < guard) | (np.abs(t - L) < guard)
    ok = (t >= -1.0) & (t <= L)
    if force == "in":
        ok = ok | near
    elif force == "out":
        ok = ok & ~near
    tc = np.maximum(t, 0.0)
    i0 = np.floor(tc).astype(np.int64)
    top = i0 >= L - 1
    i0 = np.where(top, L - 1, i0)
    i1 = np.where(top, L - 1, i0 + 1)
    w1 = np.where(top, 0.0, tc - i0)
    return t, ok, near, i0, i1, 1.0 - w1, w1


def _dyadic_q(a, qmax=40):
    """Smallest q with every element of a a multiple of 2^-q (qmax + 1 if there is none up to qmax)."""
    a = np.abs(np.asarray(a, dtype=np.float64).ravel())
    a = a[a != 0]
    for q in range(qmax + 1):
        s = np.ldexp(a, q)
        if np.array_equal(s, np.rint(s)):
            return q
    return qmax + 1


def _scatter_add(dst, idx, vals):
    """dst[idx[i]] += vals[i] (rows), duplicates included: sort + segment sums instead of np.add.at."""
    if idx.size == 0:
        return
    order = np.argsort(idx, kind="stable")
    idx, vals = idx[order], vals[order]
    starts = np.flatnonzero(np.r_[True, idx[1:] != idx[:-1]])
    dst[idx[starts]] += np.add.reduceat(vals, starts, axis=0)


def _roi_geometry(rois, scale, P, sr, aligned, guard):
    r = np.asarray(rois, dtype=np.float32).astype(np.float64)
    s = float(np.float32(scale))
    off = 0.5 if aligned else 0.0
    x1, y1, x2, y2 = (r[:, i] * s - off for i in (1, 2, 3, 4))
    rw, rh = x2 - x1, y2 - y1
    raw = np.stack([rh, rw], 1)
    if not aligned:
        rw, rh = np.maximum(rw, 1.0), np.maximum(rh, 1.0)
    bh, bw = rh / P, rw / P
    K = r.shape[0]
    if sr > 0:
        grid = np.full((K, 2), sr, dtype=np.int64)
        alt = grid.copy()
    else:
        v = np.stack([bh, bw], 1)
        grid = np.ceil(v).astype(np.int64)
        n = np.rint(v)
        amb = np.abs(v - n) < guard
        alt = np.where(amb, np.where(grid == n, n + 1, n), grid).astype(np.int64)
    return dict(b=r[:, 0].astype(np.int64), x1=x1, y1=y1, bw=bw, bh=bh, grid=grid, grid_alt=alt, raw=raw)


def _roi_level(F, G, S, geo, sel, P, gh, gw, guard, force, gout, res, exact, lv):
    """RoIs `sel` (indices into the call's RoI list; all of level lv, all with the grid gh x gw); geo holds their geometry.
    F [N, H, W, C] float64 features (forward) or None; G, S [N*H*W, C] gradient / error-scale accumulators (backward)."""
    N, H, W, C = res["shape"]
    K = sel.size
    cnt = float(max(gh * gw, 1))
    ty, oky, ny, Y0, Y1, hy, ly = _roi_axis(geo["y1"], geo["bh"], P, max(gh, 0), H, guard, force)
    tx, okx, nx, X0, X1, hx, lx = _roi_axis(geo["x1"], geo["bw"], P, max(gw, 0), W, guard, force)
    for j, k in enumerate(sel):
        res["y"][k], res["x"][k] = ty[j], tx[j]
    if gh <= 0 or gw <= 0:
        return
    R, Q = P * gh, P * gw
    ok = oky[:, :, None] & okx[:, None, :]
    res["near"][sel] |= (ny[:, :, None] | nx[:, None, :]).reshape(K, P, gh, P, gw).any(axis=(2, 4))
    b = geo["b"][:, None, None]
    corners = [(Y0, hy, X0, hx), (Y0, hy, X1, lx), (Y1, ly, X0, hx), (Y1, ly, X1, lx)]
    if F is not None:
        acc = np.zeros((K, R, Q, C))
        mag = np.zeros((K, R, Q, C))
        tot = np.zeros((K, R, Q, C))
        for Ya, wy, Xb, wx in corners:
            v = F[b, Ya[:, :, None], Xb[:, None, :]]
            w = (wy[:, :, None] * wx[:, None, :] * ok)[..., None]
            acc += w * v
            np.maximum(mag, np.abs(v) * ok[..., None], out=mag)
            if exact is not None:
                exact["q_fwd"] = max(exact["q_fwd"], _dyadic_q(w) + exact["q_feat"])      # >= that of the products
                tot += np.abs(w * v)
        bins = lambda a, f: f(a.reshape(K, P, gh, P, gw, C), axis=(2, 4)).transpose(0, 3, 1, 2)    # noqa: E731
        res["out"][sel] = bins(acc, np.sum) / cnt
        res["scale"][sel] = bins(mag, np.max)
        if exact is not None:
            exact["sum_fwd"] = max(exact["sum_fwd"], float(bins(tot, np.sum).max()))
    if G is not None:
        go = np.asarray(gout)[sel].astype(np.float64).transpose(0, 2, 3, 1) / cnt                  # [K, P, P, C]
        go = np.broadcast_to(go[:, :, None, :, None, :], (K, P, gh, P, gw, C)).reshape(K, R, Q, C)
        q_go = _dyadic_q(go[:, ::gh, ::gw]) if exact is not None else 0
        for n, (Ya, wy, Xb, wx) in enumerate(corners):
            idx = ((b * H + Ya[:, :, None]) * W + Xb[:, None, :]).reshape(-1)
            w = (wy[:, :, None] * wx[:, None, :] * ok)[..., None]
            _scatter_add(G, idx, (w * go).reshape(-1, C))
            # the scale counts a sample once per cell it touches: the repeated last row / column is one cell
            touch = ok.copy()
            if n >= 2:
                touch &= (Y1 != Y0)[:, :, None]
            if n % 2:
                touch &= (X1 != X0)[:, None, :]
            _scatter_add(S, idx, (np.abs(go) * touch[..., None]).reshape(-1, C))
            if exact is not None:
                exact["q_bwd"] = max(exact["q_bwd"], _dyadic_q(w) + q_go)
                _scatter_add(exact["cells"][lv], idx, np.abs(w * go).reshape(-1, C))


def _roi_run(feats, shapes, gout, rois, scale, pooled, sampling_ratio, aligned, level, guard, force, grid, exact):
    single = level is None
    scales = [scale] if np.isscalar(scale) else list(scale)
    rois = np.asarray(rois, dtype=np.float32).reshape(-1, 5)
    K, P = rois.shape[0], int(pooled)
    lvl = np.zeros(K, dtype=np.int64) if single else np.clip(np.asarray(level, dtype=np.int64), 0, len(shapes) - 1)
    C = shapes[0][1]
    res = dict(out=np.zeros((K, C, P, P)), scale=np.zeros((K, C, P, P)), near=np.zeros((K, P, P), dtype=bool),
               y=[None] * K, x=[None] * K, grid=np.zeros((K, 2), dtype=np.int64), grid_alt=np.zeros((K, 2), dtype=np.int64),
               raw=np.zeros((K, 2)), grad=[], gscale=[])
    ex = None
    if exact:
        ex = dict(q_fwd=0, q_feat=0, sum_fwd=0.0, q_bwd=0, q_geom=0, max_coord=0.0, cells=[np.zeros((s[0] * s[2] * s[3], C)) for s in shapes])
        res["exact"] = ex
    for lv, shape in enumerate(shapes):
        N, _, H, W = shape
        res["shape"] = (N, H, W, C)
        F = None if feats is None else np.ascontiguousarray(np.asarray(feats[lv], dtype=np.float32).astype(np.float64).transpose(0, 2, 3, 1))
        if ex is not None and F is not None:
            ex["q_feat"] = _dyadic_q(F)
        G = S = None
        if gout is not None:
            G, S = np.zeros((N * H * W, C)), np.zeros((N * H * W, C))
        here = np.flatnonzero(lvl == lv)
        if here.size:
            geo = _roi_geometry(rois[here], scales[lv], P, sampling_ratio, aligned, guard)
            res["grid"][here], res["grid_alt"][here], res["raw"][here] = geo["grid"], geo["grid_alt"], geo["raw"]
            res["near"][here[(geo["grid"] != geo["grid_alt"]).any(axis=1)]] = True
            if ex is not None:
                g = np.concatenate([geo[k] for k in ("x1", "y1", "bw", "bh")])
                ex["q_geom"] = max(ex["q_geom"], _dyadic_q(g))
                ex["max_coord"] = max(ex["max_coord"], float(np.abs(g).max()))
            use = geo["grid"] if grid is None else np.asarray(grid, dtype=np.int64)[here]
            for gh, gw in sorted(set(map(tuple, use.tolist()))):
                loc = np.flatnonzero((use[:, 0] == gh) & (use[:, 1] == gw))
                step = max(1, int(4e6 // (P * P * max(gh, 1) * max(gw, 1) * C)))
                for s0 in range(0, loc.size, step):
                    part = loc[s0:s0 + step]
                    _roi_level(F, G, S, {k: v[part] for k, v in geo.items()}, here[part], P, gh, gw, guard, force, gout, res, ex, lv)
        if gout is not None:
            res["grad"].append(G.reshape(N, H, W, C).transpose(0, 3, 1, 2))
            res["gscale"].append(S.reshape(N, H, W, C).transpose(0, 3, 1, 2))
    if ex is not None:
        ex["sum_bwd"] = max(float(c.max()) if c.size else 0.0 for c in ex["cells"])
        del ex["cells"]
    del res["shape"]
    if gout is None:
        del res["grad"], res["gscale"]
    elif single:
        res["grad"], res["gscale"] = res["grad"][0], res["gscale"][0]
    return res


def roi_align64(feat, rois, scale, pooled, sampling_ratio, aligned, level=None, guard=0.0, force="ref", grid=None,
                exact=False):
    """RoIAlign as defined above.  feat [N, C, H, W] float32 with a scalar scale, or a list of levels with a list of
    scales and `level` [K] (the level each RoI pools from).  Returns a dict:
      out    [K, C, P, P] float64;
      near   [K, P, P] bool -- the bin has a sample within `guard` of y = -1, y = H, x = -1 or x = W (the only points where
             the definition is discontinuous in the coordinates) or, with adaptive sampling, the RoI's grid != grid_alt;
      scale  [K, C, P, P] -- the largest |feature value| the element's samples touch (its error scale);
      y, x   per RoI, the float64 sample coordinates of the two axes (P * gh and P * gw of them);
      grid   [K, 2] (gh, gw);  grid_alt [K, 2]: where size / P lies within `guard` of an integer, the other grid size a
             float32 evaluation may arrive at (equal to grid elsewhere);  raw [K, 2]: (height, width) before the clamp.
    force = "in" / "out" evaluates the samples within the guard as inside / outside; grid = [K, 2] overrides the grid.
    exact=True adds `exact`: q_fwd with every term weight * feature a multiple of 2^-q_fwd (the smallest such q of the
    weights plus that of the features), the largest
    sum of |terms| of one output (sum_fwd), and q_geom / max_coord for the RoI geometry."""
    feats = [feat] if level is None else list(feat)
    shapes = [tuple(np.asarray(f).shape) for f in feats]
    return _roi_run(feats, shapes, None, rois, scale, pooled, sampling_ratio, aligned, level, guard, force, grid, exact)


def roi_align_backward64(gout, shape, rois, scale, pooled, sampling_ratio, aligned, level=None, guard=0.0, force="ref",
                         grid=None, exact=False):
    """The transpose of roi_align64: gout [K, C, P, P] -> grad [N, C, H, W] float64 (a list with `level`); `shape` is the
    feature shape (a list of shapes with `level`).  Also `gscale`, per feature cell the sum of |gout| / count over the
    samples that touch it (unweighted: a weight near 0 still carries the absolute coordinate error), and with
    exact=True q_bwd / sum_bwd: the terms weight * gout / count and their largest sum of magnitudes per feature cell."""
    shapes = [tuple(shape)] if level is None else [tuple(s) for s in shape]
    return _roi_run(None, shapes, gout, rois, scale, pooled, sampling_ratio, aligned, level, guard, force, grid, exact)


def nms_greedy(boxes, valid, thr):
    """Greedy NMS over integer-coordinate boxes [n, 4] (x1, y1, x2, y2) given in score order; valid [n] bool or None.
    Returns the kept positions.  Box i, once kept, removes every later j with IoU(i, j) > thr; an invalid box is never
    kept and never removes.  The decision is made on exact integers:
      inter = max(min(x2) - max(x1), 0) * max(min(y2) - max(y1), 0), union = area_i + area_j - inter, area = (x2 - x1) *
      (y2 - y1) unclamped as in torchvision's box_iou (a box with two negative sides has a positive area);
      inter == 0 never removes: 0 / union is 0, -0 or (zero-area boxes, 0 / 0) NaN, and none of them is > thr >= 0;
      inter > 0 means both boxes have positive sides, so union > 0: thr = 0.5 decides by 2 * inter > union, any other
      threshold by the one correctly rounded division float32(inter) / float32(union) > float32(thr)."""
    b = np.asarray(boxes)
    assert np.array_equal(b, np.rint(b)) and thr >= 0
    b = b.astype(np.int64)
    n = b.shape[0]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    assert n == 0 or (np.abs(b).max() < 2 ** 24 and np.abs(area).max() < 2 ** 23), "every float32 step must be exact"
    removed = np.zeros(n, dtype=bool) if valid is None else ~np.asarray(valid, dtype=bool)
    keep = []
    t32 = np.float32(thr)
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        r = b[i + 1:]
        iw = np.minimum(b[i, 2], r[:, 2]) - np.maximum(b[i, 0], r[:, 0])
        cand = np.flatnonzero(iw > 0)
        if cand.size == 0:
            continue
        r = r[cand]
        ih = np.minimum(b[i, 3], r[:, 3]) - np.maximum(b[i, 1], r[:, 1])
        inter = iw[cand] * np.maximum(ih, 0)
        union = area[i] + area[i + 1:][cand] - inter
        pos = inter > 0
        assert (union[pos] > 0).all() and (union[pos] < 2 ** 24).all()
        if thr == 0.5:
            sup = pos & (2 * inter > union)
        else:
            sup = pos & (inter.astype(np.float32) / np.where(pos, union, 1).astype(np.float32) > t32)
        removed[i + 1 + cand[sup]] = True
    return keep


# --------------------------------------------------------------------------------------
# A20 box matching, coding and detection candidates: float64 / int64 references for csrc/dib_detect.hip
#     (torchvision's box_iou / Matcher / BoxCoder / RoIHeads.postprocess_detections up to the NMS, which reference
#     models/faster_rcnn.py:150-159,198-229 configures)
# --------------------------------------------------------------------------------------
# Written from the published definitions in numpy float64 / int64, not from the kernels and without torch.  Boxes are
# (x1, y1, x2, y2) float32 and are widened before the first operation.

def _boxes64(b):
    return np.asarray(b, dtype=np.float32).astype(np.float64).reshape(-1, 4)


def box_iou64(gt, cand):
    """[G, 4] x [M, 4] -> [G, M] float64: inter / (area_a + area_b - inter) with the intersection's sides clamped at 0
    and the areas unclamped (torchvision's box_iou); 0 / 0 is NaN."""
    a, b = _boxes64(gt), _boxes64(cand)
    lt = np.maximum(a[:, None, :2], b[None, :, :2])
    rb = np.minimum(a[:, None, 2:], b[None, :, 2:])
    wh = np.maximum(rb - lt, 0.0)
    inter = wh[..., 0] * wh[..., 1]
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / (area_a[:, None] + area_b[None, :] - inter)


def _max_first(q, axis):
    """(max, argmax) along `axis` as torch.max: the first index on ties (-0 == 0), the first NaN when there is one."""
    nan = np.isnan(q)
    has = nan.any(axis=axis)
    arg = np.where(has, nan.argmax(axis=axis), np.where(nan, -np.inf, q).argmax(axis=axis))
    return np.take_along_axis(q, np.expand_dims(arg, axis), axis).squeeze(axis), arg


def match64(gt, cand, high, low, allow_low, guard=0.0):
    """torchvision's Matcher on box_iou64 for one image: match [M] int64 -- the index of the ground truth of highest IoU,
    -1 where that IoU is < low, -2 where it is in [low, high); with allow_low every candidate that attains some ground
    truth's best IoU keeps its own argmax (a best of 0 restores every candidate with IoU 0).  No ground truth: -1.

    guard == 0: the IoU is rounded once to float32 and the thresholds are np.float32(thr) -- for inputs whose areas,
    intersections and unions are integers below 2^24 that is the float32 IoU of any correct implementation, and the
    result is THE answer.  NaN (0 / 0) wins a candidate's maximum once and propagates into a ground truth's best, where
    it equals nothing.

    guard > 0: returns (match, accept [M, G + 2] bool -- accept[m, v + 2] says that answer v is acceptable --, near [M]).
    Decisions are taken on the float64 IoU; an answer is acceptable when an IoU error below `guard` can produce it:
    the maximum within guard of a threshold (both classes), a second ground truth within guard of the maximum (either
    index), a candidate within guard of a ground truth's best without being its unique clear maximum (restored or
    not).  Equal float64 IoUs of identical boxes, and IoUs that are exactly 0, are ties in float32 as well: the lowest
    index / every such candidate is required, and they are not `near`."""
    g32, c32 = np.asarray(gt, dtype=np.float32).reshape(-1, 4), np.asarray(cand, dtype=np.float32).reshape(-1, 4)
    G, M = len(g32), len(c32)
    lo, hi = float(np.float32(low)), float(np.float32(high))
    if G == 0:
        match = np.full(M, -1, dtype=np.int64)
        if guard <= 0:
            return match
        accept = np.zeros((M, 2), dtype=bool)
        accept[:, 1] = True
        return match, accept, np.zeros(M, dtype=bool)
    q = box_iou64(g32, c32)
    if guard <= 0:
        q = q.astype(np.float32).astype(np.float64)
    cols = np.arange(M)
    with np.errstate(invalid="ignore"):
        vals, arg = _max_first(q, 0)
        match = arg.astype(np.int64)
        match[vals < lo] = -1
        match[(vals >= lo) & (vals < hi)] = -2
        if allow_low:
            best, _ = _max_first(q, 1)
            match = np.where((q == best[:, None]).any(axis=0), arg, match)
        if guard <= 0:
            return match
        # ---- the acceptable set
        has_nan = np.isnan(vals)
        qq = np.where(np.isnan(q), -np.inf, q)
        vmax = qq.max(axis=0)
        S = qq >= vmax[None, :] - guard                               # indices a float32 argmax may return
        same_gt = (g32[:, None, :] == g32[None, :, :]).all(axis=2)
        for g in range(1, G):                                         # true ties: the lower index always wins
            tie = S[:g] & (qq[:g] == qq[g][None, :]) & (same_gt[:g, g][:, None] | (qq[g] == 0)[None, :])
            S[g] &= ~tie.any(axis=0)
        S[:, has_nan] = False
        S[arg[has_nan], cols[has_nan]] = True                         # 0 / 0 is NaN in any precision: decisive
        multi = S.sum(axis=0) > 1
        may_below = (vmax < lo + guard) & ~has_nan
        may_between = (vmax >= lo - guard) & (vmax < hi + guard) & (hi > lo) & ~has_nan
        may_match = (vmax >= hi - guard) | has_nan
        sure = np.zeros(M, dtype=bool)
        maybe = np.zeros(M, dtype=bool)
        if allow_low:
            bestq = np.where(np.isnan(best), np.inf, best)            # a NaN best equals nothing
            T = qq >= bestq[:, None] - guard
            first = T.argmax(axis=1)
            same_c = (c32[None, :, :] == c32[first][:, None, :]).all(axis=2)
            clean = ((~T | ((qq == bestq[:, None]) & (same_c | (bestq == 0)[:, None]))).all(axis=1)) & T.any(axis=1)
            sure = (T & clean[:, None]).any(axis=0)
            maybe = (T & ~clean[:, None]).any(axis=0) & ~sure
        accept = np.zeros((M, G + 2), dtype=bool)
        base_idx = may_match | sure | maybe
        accept[:, 2:] = (S & base_idx[None, :]).T
        accept[:, 1] = may_below & ~sure
        accept[:, 0] = may_between & ~sure
        n_class = may_below.astype(int) + may_between + may_match
        near = maybe | (~sure & (n_class > 1)) | (multi & base_idx)
    return match, accept, near


def box_encode64(ref, cand, weights):
    """R-CNN parameterisation of `ref` [M, 4] against `cand` [M, 4] in float64: (targets [M, 4], scale [M, 4]) with
    dx = wx (gx - px) / pw, dw = ww log(gw / pw) (centres x + w / 2) and, per element, the magnitude a float32 rounding
    error is relative to: wx (|gx| + |px|) / pw for the centres, ww (1 + |log(gw / pw)|) for the sizes."""
    r, p = _boxes64(ref), _boxes64(cand)
    wx, wy, ww, wh = [float(v) for v in weights]
    out, scale = np.empty((len(p), 4)), np.empty((len(p), 4))
    with np.errstate(divide="ignore", invalid="ignore"):
        for k, (wc, ws) in enumerate(((wx, ww), (wy, wh))):
            ps, gs = p[:, 2 + k] - p[:, k], r[:, 2 + k] - r[:, k]
            pc, gc = p[:, k] + 0.5 * ps, r[:, k] + 0.5 * gs
            out[:, k] = wc * (gc - pc) / ps
            scale[:, k] = wc * (np.abs(gc) + np.abs(pc)) / np.abs(ps)
            out[:, 2 + k] = ws * np.log(gs / ps)
            scale[:, 2 + k] = ws * (1.0 + np.abs(np.log(gs / ps)))
    return out, scale


def _decode64(d, b, weights, clip):
    """d [..., 4] deltas against b [..., 4] boxes (broadcast), float64 -> boxes, scale."""
    wx, wy, ww, wh = [float(v) for v in weights]
    out, scale = np.empty(d.shape), np.empty(d.shape)
    with np.errstate(over="ignore", invalid="ignore"):
        for k, (wc, ws) in enumerate(((wx, ww), (wy, wh))):
            size = b[..., 2 + k] - b[..., k]
            c = b[..., k] + 0.5 * size
            dc, ds = d[..., k] / wc, d[..., 2 + k] / ws
            ds = np.where(ds > clip, clip, ds)                        # min(dw, clip): NaN stays NaN
            pc, ps = dc * size + c, np.exp(ds) * size
            out[..., k], out[..., 2 + k] = pc - 0.5 * ps, pc + 0.5 * ps
            s = np.abs(c) + np.abs(dc) * np.abs(size) + np.abs(ps) * (1.0 + np.abs(ds))
            scale[..., k], scale[..., 2 + k] = s, s
    return out, scale


DECODE_CLIP = float(np.float32(math.log(1000.0 / 16)))


def box_decode64(deltas, anchors, weights, clip=DECODE_CLIP):
    """The inverse: deltas [R, 4] against anchors [A, 4] (row r uses anchor r % A) -> (boxes [R, 4], scale [R, 4]) in
    float64, with true division by the weights and min(dw, clip), clip = float32(log(1000 / 16)) widened; the scale of
    both corners of an axis is |cx| + |dx| w + pw (1 + |dw|)."""
    d = np.asarray(deltas, dtype=np.float32).astype(np.float64).reshape(-1, 4)
    a = _boxes64(anchors)
    return _decode64(d, a[np.arange(len(d)) % len(a)], weights, float(clip))


def det_candidates64(logits, deltas, rois, shape, weights, clip, score_thresh, min_size, c_score=0.0, c_box=0.0):
    """One image's detection candidates before the NMS, class-major as the kernel writes them (class c in row c - 1):
    logits [R, C], deltas [R, 4 C], rois [R, 4], shape (h, w) -> dict with
      scores [C - 1, R] the float64 softmax,         sscale = score (1 + |x - max|) + 2^-126,
      boxes [C - 1, R, 4] decoded and clipped,       bscale as box_decode64 (clipping is 1-Lipschitz),
      kept: score > float32(score_thresh) and both sides >= float32(min_size),
      near: the score is within c_score 2^-24 sscale of the threshold, or a side computed from corners that are each
            off by up to c_box 2^-24 bscale (and then clipped) can fall on either side of min_size."""
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    R, C = x.shape
    d = np.asarray(deltas, dtype=np.float32).astype(np.float64).reshape(R, C, 4)
    m = x.max(axis=1, keepdims=True)
    e = np.exp(x - m)
    s = e / e.sum(axis=1, keepdims=True)
    sscale = s * (1.0 + np.abs(x - m)) + 2.0 ** -126
    raw, bscale = _decode64(d, _boxes64(rois)[:, None, :], weights, float(clip))
    h, w = float(shape[0]), float(shape[1])
    hi = np.array([w, h, w, h])

    def clipped(v):
        v = np.where(v < 0, 0.0, v)
        return np.where(v > hi, hi, v)                                 # NaN stays NaN
    boxes = clipped(raw)
    thr, mins = float(np.float32(score_thresh)), float(np.float32(min_size))
    u = 2.0 ** -24
    with np.errstate(invalid="ignore"):
        sides = boxes[..., 2:] - boxes[..., :2]
        kept = (s > thr) & (sides >= mins).all(axis=-1)
        eb = c_box * u * bscale
        side_lo = clipped(raw - eb)[..., 2:] - clipped(raw + eb)[..., :2]
        side_hi = clipped(raw + eb)[..., 2:] - clipped(raw - eb)[..., :2]
        near_side = ((side_lo < mins) & (side_hi >= mins)).any(axis=-1)
        near = (np.abs(s - thr) <= c_score * u * sscale) | near_side
    cm = lambda a: np.ascontiguousarray(np.moveaxis(a[:, 1:], 0, 1))
    return dict(scores=cm(s), sscale=cm(sscale), boxes=cm(boxes), bscale=cm(bscale), kept=cm(kept), near=cm(near))


def pool64(props, gts, g_pad):
    """box_pool_kernel: props [N, P, 4] -> [N, P + g_pad, 4] float32, image n's proposals, then its ground truth, then
    [0, 0, 1, 1] rows."""
    props = np.asarray(props, dtype=np.float32)
    N, P = props.shape[:2]
    out = np.empty((N, P + g_pad, 4), dtype=np.float32)
    out[:, :P] = props
    out[:, P:] = np.array([0, 0, 1, 1], dtype=np.float32)
    for n, g in enumerate(gts):
        assert len(g) <= g_pad
        out[n, P:P + len(g)] = np.asarray(g, dtype=np.float32).reshape(-1, 4)
    return out


def labels64(match, gt_labels, ok, P):
    """box_labels_kernel: match [N, M] int64 -> labels [N, M] int64: gt_labels[n][match] for match >= 0 (index clamped to
    the image's last ground truth; 0 for an image without any), 0 for -1, -1 for -2; -1 on rows that are padding
    (proposal rows j < P with ok[n, j] == 0, ground-truth rows j - P beyond the image's count)."""
    match = np.asarray(match, dtype=np.int64)
    N, M = match.shape
    out = np.empty((N, M), dtype=np.int64)
    j = np.arange(M)
    for n in range(N):
        lab = np.asarray(gt_labels[n], dtype=np.int64)
        G = len(lab)
        got = lab[np.clip(match[n], 0, G - 1)] if G else np.zeros(M, dtype=np.int64)
        v = np.where(match[n] >= 0, got, np.where(match[n] == -1, 0, -1))
        live = j - P < G
        live[:P] = True if ok is None else np.asarray(ok)[n, :P] != 0
        out[n] = np.where(live, v, -1)
    return out


# --------------------------------------------------------------------------------------
# A21 trunk epilogues: float32 references for csrc/dib_eltwise_vec.h (both lane types), the scalar and the transposing
#     kernel of csrc/dib_eltwise.hip and the apply pass of csrc/dib_bnstats.hip
#     (torchvision's Bottleneck / FeaturePyramidNetwork / ResNet stem arithmetic between the convolutions, which
#     reference models/faster_rcnn.py:367 builds)
# --------------------------------------------------------------------------------------
# Plain numpy on the host, no torch, nothing of the package.  Activations are channels-last arrays [N, H, W, C] (or flat, channel
# fastest) of float32; every addition is ONE float32 operation in the kernels' documented order, so a correct kernel equals
# these bit for bit (NaN by position).  tests/test_trunk_epilogue_reference.py holds them to torch on the CPU.

def relu32(v):
    """torch's relu in values -- a NaN goes through -- with the kernels' zero: every result that is not > 0 and not NaN is +0.0
    (torch.relu on the CPU returns -0.0 for -0.0)."""
    v = np.asarray(v)
    return np.where((v > 0) | np.isnan(v), v, v.dtype.type(0.0))


def bias_act32(x, bias, res=None, relu=False):
    """bias_act_kernel / bias_act_scalar_kernel: act((x + bias[c]) + res)."""
    with np.errstate(invalid="ignore", over="ignore"):                     # inf - inf is data here
        v = np.asarray(x, dtype=np.float32) + np.asarray(bias, dtype=np.float32)
        if res is not None:
            v = v + np.asarray(res, dtype=np.float32)
    return relu32(v) if relu else v


def sign_mask(y, lane=4):
    """The ReLU mask: one byte per `lane` consecutive stored elements (4 for fp32, 8 for bf16), bit k = element k > 0.  A NaN
    carries no bit."""
    bits = (np.asarray(y).reshape(-1, lane) > 0).astype(np.uint32)
    return (bits << np.arange(lane, dtype=np.uint32)).sum(1).astype(np.uint8)


def mask_bits(mask, lane=4):
    """sign_mask's inverse: a flat bool array, one entry per element."""
    return ((np.asarray(mask, dtype=np.uint8)[:, None] >> np.arange(lane, dtype=np.uint8)) & 1).astype(bool).reshape(-1)


def mask_select(g, mask, lane=4):
    """relu_mask_bwd_kernel: mask ? g : +0.0."""
    g = np.asarray(g)
    return np.where(mask_bits(mask, lane).reshape(g.shape), g, g.dtype.type(0.0))


def add_relu_mask32(a, b, mask=None):
    """add_mask_kernel: a + b, then cleared (+0.0) where the mask bit is clear; no mask: the plain sum."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.asarray(a, dtype=np.float32) + np.asarray(b, dtype=np.float32)
    return s if mask is None else mask_select(s, mask)


def scatter_add32(a, b, stride):
    """scatter_add_kernel: a[n, ys * stride, xs * stride, :] += b[n, ys, xs, :]; every other element of a unchanged."""
    out = np.array(a, dtype=np.float32, copy=True)
    Hs, Ws = b.shape[1], b.shape[2]
    with np.errstate(invalid="ignore", over="ignore"):
        out[:, 0:(Hs - 1) * stride + 1:stride, 0:(Ws - 1) * stride + 1:stride, :] += np.asarray(b, dtype=np.float32)
    return out


def nearest_src(out_size, in_size):
    """ATen's nearest-neighbour source index (upsample_nearest2d with an output size): min(int(floorf(dst * scale)), in - 1)
    with scale = float32(in) / float32(out), the product in float32."""
    scale = np.float32(in_size) / np.float32(out_size)
    dst = np.arange(out_size, dtype=np.float32)
    return np.minimum(np.floor(dst * scale).astype(np.int64), in_size - 1)


def topdown_merge32(x, bias, top):
    """topdown_merge_kernel: (x + bias[c]) + top[n, sh(h), sw(w), :]."""
    H, W = x.shape[1], x.shape[2]
    sh, sw = nearest_src(H, top.shape[1]), nearest_src(W, top.shape[2])
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(x, dtype=np.float32) + np.asarray(bias, dtype=np.float32)
        return v + np.asarray(top, dtype=np.float32)[:, sh][:, :, sw]


def stem_pool32(x, bias):
    """stem_pool_fwd_kernel: relu32(x + bias), then the 3 x 3 / stride 2 / padding 1 maximum with ATen's selection: the first
    maximum in row-major window order wins, a NaN beats everything and the LAST NaN of a window wins.  Returns the pooled values
    [N, Ho, Wo, C] float32 and the winner's window position 0..8 (uint8; 15 where the maximum is not > 0 and not NaN: no
    gradient)."""
    with np.errstate(invalid="ignore", over="ignore"):
        y = relu32(np.asarray(x, dtype=np.float32) + np.asarray(bias, dtype=np.float32))
    N, H, W, C = y.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pad = np.full((N, 2 * Ho + 2, 2 * Wo + 2, C), -np.inf, dtype=np.float32)
    pad[:, 1:H + 1, 1:W + 1] = y
    m = np.full((N, Ho, Wo, C), -np.inf, dtype=np.float32)
    pos = np.full((N, Ho, Wo, C), 15, dtype=np.uint8)
    for k in range(9):
        v = pad[:, k // 3:k // 3 + 2 * Ho:2, k % 3:k % 3 + 2 * Wo:2]
        take = (v > m) | np.isnan(v)
        m = np.where(take, v, m)
        pos = np.where(take, np.uint8(k), pos)
    dead = ~(m > 0) & ~np.isnan(m)
    return np.where(dead, np.float32(0.0), m), np.where(dead, np.uint8(15), pos)


def pack_pool_arg(pos):
    """The kernels' `arg`: one uint16 per 4 consecutive channels, 4 bits per channel, channel 4 i in the low nibble."""
    p = np.asarray(pos, dtype=np.uint16).reshape(-1, 4)
    return (p[:, 0] | (p[:, 1] << 4) | (p[:, 2] << 8) | (p[:, 3] << 12)).astype(np.uint16)


def stem_pool_backward64(gout, pos, H, W):
    """stem_pool_bwd_kernel: the pooled gradient goes to the recorded position (none for 15); an input pixel sums the at most
    four windows it won, here in float64."""
    gout = np.asarray(gout, dtype=np.float64)
    N, Ho, Wo, C = gout.shape
    pad = np.zeros((N, 2 * Ho + 2, 2 * Wo + 2, C), dtype=np.float64)
    for k in range(9):
        pad[:, k // 3:k // 3 + 2 * Ho:2, k % 3:k % 3 + 2 * Wo:2] += np.where(pos == k, gout, 0.0)
    return pad[:, 1:H + 1, 1:W + 1]


def to_bf16_bits(v):
    """float32 -> bfloat16 bit patterns (uint16), round to nearest even; NaN stays NaN, +-inf stays."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return np.where(np.isnan(v), np.uint16(0x7FC0), r)


def from_bf16_bits(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


# --------------------------------------------------------------------------------------
# A23 the detector's and estimator's input transform: float64 / IEEE float32 reference for csrc/dib_epilogue.hip
#     (normalize_pad_kernel, normalize_resize_pad_kernel behind dib_normalize_pad / dib_normalize_resize_pad /
#     dib_normalize_resize_crop; reference engine.py:107-110, models/net_transforms.py:112-121, :151-175, :226-247,
#     engine_blur_estimator.py:217)
# --------------------------------------------------------------------------------------
# Plain numpy on the host, no torch, nothing of the package.  What is exact in the kernels is stated exactly: the normalised source
# pixel (two correctly rounded float32 operations), the sampling position and its weights (float32), the quantisation, the
# padding.  The one approximate stage, the four-term interpolation, is evaluated in float64 from those float32 operands, and the
# magnitude the error bound scales with is returned with it.  tests/test_input_transform_reference.py holds this section to torch
# on the CPU and to tests/golden/net_transforms.npz.

TRANSFORM_UNIT = 2.0 ** -24            # half an ulp of a float32 in [1, 2): one rounding of a value of magnitude <= 1
TRANSFORM_BOUND = 5.0                  # in units of TRANSFORM_UNIT * M: product, inner sum, outer product, outer sum, each at most one
                                       # unit of a magnitude the convex weights keep <= M, and one for the second-order terms; the
                                       # contracted form has fewer roundings


def transform_quantize(x):
    """`(img * 255).type(torch.uint8).type(torch.half) / 255` as ATen evaluates it on Half: a = half(float(x) * 255f),
    k = uint8(trunc(a)), q = half(float(k) / 255f).  Domain: finite x >= 0 with half(x * 255) < 256."""
    x = np.asarray(x, dtype=np.float16)
    a = (x.astype(np.float32) * np.float32(255.0)).astype(np.float16)
    if not (np.isfinite(x) & (x >= 0) & (a < 256)).all():
        raise ValueError("transform_quantize: outside the documented domain")
    k = np.trunc(a.astype(np.float32)).astype(np.uint8)
    return (k.astype(np.float32) / np.float32(255.0)).astype(np.float16)


def transform_normalize(image, mean, std, quantize=False):
    """[3, H, W] float16 / float32 -> float32 n = (float32(p) - mean32) / std32, each operation ONE float32 rounding."""
    image = np.asarray(image)
    if image.dtype not in (np.float16, np.float32) or image.ndim != 3 or image.shape[0] != 3:
        raise ValueError("transform_normalize: 3 x H x W float16 / float32 images")
    if quantize:
        image = transform_quantize(image)
    m = np.asarray(mean, dtype=np.float64).astype(np.float32).reshape(3, 1, 1)
    s = np.asarray(std, dtype=np.float64).astype(np.float32).reshape(3, 1, 1)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return (image.astype(np.float32) - m) / s


def transform_positions(n_in, n_out, contracted=True):
    """One axis of the bilinear resize (align_corners=False, the scale recomputed from the integer sizes).  Returns
    (i, ip, l0, l1, s): the first source index, whether a second one follows it (the edge clamp), the float32 weights of the two
    exactly as the kernel forms them, and the real-arithmetic position s = (n_in / n_out)(dst + 0.5) - 0.5 clamped to
    [0, n_in - 1] in float64.  r32 * (dst + 0.5) is exact in float64, so `contracted` (the kernel's fmaf, ATen's arithmetic on the
    GPU) is one rounding of r32 * (dst + 0.5) - 0.5; the uncontracted form rounds the product first."""
    r32 = np.float32(n_in) / np.float32(n_out)
    t = np.arange(n_out, dtype=np.float64) + 0.5
    if contracted:
        s32 = (np.float64(r32) * t - 0.5).astype(np.float32)
    else:
        s32 = (np.float64(r32) * t).astype(np.float32) - np.float32(0.5)
    s32 = np.where(s32 < 0, np.float32(0.0), s32).astype(np.float32)
    i = s32.astype(np.int64)
    ip = (i < n_in - 1).astype(np.int64)
    l1 = s32 - i.astype(np.float32)                       # exact
    l0 = np.float32(1.0) - l1
    s = np.clip((np.float64(n_in) / np.float64(n_out)) * t - 0.5, 0.0, float(n_in - 1))
    return i, ip, l0, l1, s


def _real_positions(n_in, n_out):
    s = transform_positions(n_in, n_out)[4]
    i = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    return i, (i < n_in - 1).astype(np.int64), 1.0 - (s - i), s - i


def _bilinear64(n, hpos, wpos):
    """l0h (l0w p00 + l1w p01) + l1h (l0w p10 + l1w p11) in float64, and M = max |p00, p01, p10, p11| per element."""
    n = np.asarray(n, dtype=np.float64)
    (h, hp, l0h, l1h), (w, wp, l0w, l1w) = hpos, wpos
    l0h, l1h = (np.asarray(v, dtype=np.float64).reshape(-1, 1) for v in (l0h, l1h))
    l0w, l1w = (np.asarray(v, dtype=np.float64).reshape(1, -1) for v in (l0w, l1w))
    p00, p01 = n[:, h][:, :, w], n[:, h][:, :, w + wp]
    p10, p11 = n[:, h + hp][:, :, w], n[:, h + hp][:, :, w + wp]
    with np.errstate(invalid="ignore", over="ignore"):      # 0 * inf and inf - inf are data here
        v = l0h * (l0w * p00 + l1w * p01) + l1h * (l0w * p10 + l1w * p11)
        M = np.fmax(np.fmax(np.abs(p00), np.abs(p01)), np.fmax(np.abs(p10), np.abs(p11)))
    return v, np.where(np.isnan(p00) | np.isnan(p01) | np.isnan(p10) | np.isnan(p11), np.nan, M)


def transform_bilinear_real64(n, Ho, Wo):
    """Bilinear interpolation of n [3, H, W] at the real-arithmetic positions, all in float64: what F.interpolate(mode="bilinear",
    align_corners=False, size=(Ho, Wo)) computes in float64."""
    return _bilinear64(n, _real_positions(n.shape[1], Ho), _real_positions(n.shape[2], Wo))[0]


def input_transform64(images, means, stds, out_sizes, Hp, Wp, crop=False, quantize=False, contracted=True):
    """The batch [B, 3, Hp, Wp] of dib_normalize_pad (out_sizes None), dib_normalize_resize_pad and dib_normalize_resize_crop for a
    list of 3 x H x W float16 / float32 images, per-image means / stds (rounded to float32 first), per-image (Ho, Wo).  pad: image k
    resized sits in the top-left corner, +0.0 around it; `crop`: the top-left Hp x Wp corner of every resized image.  Returns
      v      float64: for an image with (Ho, Wo) == (H, W) the float32 n itself, otherwise the interpolation in float64 from the
             float32 weights and the float32 n; +0.0 in the padding
      M      float64: max |p00, p01, p10, p11| per element (|n| at unit scale, 0 in the padding)
      exact  bool: unit-scale and padding elements, where a kernel has to give the bits of float32(v)."""
    B = len(images)
    means = np.asarray(means, dtype=np.float64).reshape(B, 3)
    stds = np.asarray(stds, dtype=np.float64).reshape(B, 3)
    v = np.zeros((B, 3, Hp, Wp), dtype=np.float64)
    M = np.zeros((B, 3, Hp, Wp), dtype=np.float64)
    exact = np.ones((B, 3, Hp, Wp), dtype=bool)
    for k, image in enumerate(images):
        n = transform_normalize(image, means[k], stds[k], quantize)
        H, W = n.shape[1:]
        Ho, Wo = (H, W) if out_sizes is None else (int(out_sizes[k][0]), int(out_sizes[k][1]))
        if crop and (Hp > Ho or Wp > Wo):
            raise ValueError("input_transform64: image %d is (resized) smaller than the crop" % k)
        if not crop and (Ho > Hp or Wo > Wp):
            raise ValueError("input_transform64: image %d is (resized) larger than the batch" % k)
        if (Ho, Wo) == (H, W):
            val, mag = n.astype(np.float64), np.abs(n.astype(np.float64))
        else:
            val, mag = _bilinear64(n, transform_positions(H, Ho, contracted)[:4], transform_positions(W, Wo, contracted)[:4])
        h, w = min(Ho, Hp), min(Wo, Wp)
        v[k, :, :h, :w], M[k, :, :h, :w] = val[:, :h, :w], mag[:, :h, :w]
        exact[k, :, :h, :w] = (Ho, Wo) == (H, W)
    return v, M, exact


def _f32_class(a):
    return np.where(np.isnan(a), 3, np.where(a == np.inf, 1, np.where(a == -np.inf, 2, 0)))


def input_transform_compare(got, v, M, exact):
    """The one comparison of a kernel's float32 batch with input_transform64's (v, M, exact).  Asserts, in order: NaN, +inf and
    -inf exactly where float32(v) has them; unit-scale and padding elements bit-equal (-0 is not +0); every other finite element
    within TRANSFORM_BOUND * 2**-24 * M of v.  Non-finite reference elements may be at most 10 % of the batch.  Returns the peak
    deviation of the bounded elements in units of 2**-24 * M."""
    got = np.ascontiguousarray(got)
    assert got.dtype == np.float32 and got.shape == v.shape == M.shape == exact.shape, (got.dtype, got.shape, v.shape)
    with np.errstate(over="ignore"):
        v32 = v.astype(np.float32)
    special = _f32_class(v32) != 0
    assert special.sum() <= 0.1 * special.size, "inputs: %d of %d reference elements are not finite" % (special.sum(), special.size)
    wrong = np.argwhere(_f32_class(got) != _f32_class(v32))
    assert len(wrong) == 0, "NaN / inf class differs at %d elements, first %s: got %r, reference %r" % (
        len(wrong), tuple(int(j) for j in wrong[0]), got[tuple(wrong[0])], v32[tuple(wrong[0])])
    sel = exact & ~special
    wrong = np.argwhere(sel & (got.view(np.uint32) != v32.view(np.uint32)))
    assert len(wrong) == 0, "unit-scale / padding bits differ at %d elements, first %s: got %r, reference %r" % (
        len(wrong), tuple(int(j) for j in wrong[0]), got[tuple(wrong[0])], v32[tuple(wrong[0])])
    sel = ~exact & ~special
    err = np.abs(got.astype(np.float64)[sel] - v[sel])
    unit = TRANSFORM_UNIT * M[sel]
    wrong = err > TRANSFORM_BOUND * unit
    if wrong.any():
        at = tuple(int(j) for j in np.argwhere(sel)[np.argmax(wrong)])
        raise AssertionError("%d elements beyond %g * 2^-24 * M, first %s: got %r, reference %r, M %r" % (
            wrong.sum(), TRANSFORM_BOUND, at, got[at], v[at], M[at]))
    live = unit > 0
    return float((err[live] / unit[live]).max()) if live.any() else 0.0
