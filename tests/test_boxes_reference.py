"""csrc/dib_detect.hip -- dib_box_match, dib_box_encode_matched, dib_box_decode, dib_box_pool, dib_box_labels and
dib_det_candidates -- against references that are more precise than the kernels (oracle/dib_oracle.py A20: numpy float64
/ int64, no torch, nothing of the package).  tests/test_detect_gpu.py and tests/test_detect_fuzz_gpu.py compare the same
kernels bit for bit with the float32 tensor expressions of models/detector_ops.py on the same device; this file is the
check that does not share their arithmetic, their device functions or their shapes.

Per entry point:
  * dib_box_match -- exact regime: integer corners in [0, 1024), so every area, intersection and union is an integer
    below 2^24 and the float32 IoU of any correct implementation is ONE correctly rounded quotient, which
    float32(i64 / u64) equals (double rounding is innocuous for a division when 53 >= 2 * 24 + 2); match64(guard = 0) is
    THE answer, bit for bit.  General regime: random float32 boxes; every answer must lie in match64's acceptable set
    with guard = 32 * 2^-24 (derivation at GUARD), at most 1 % of a case's candidates may be `near`;
  * dib_box_encode_matched -- `matched`: exact (a gather; both regimes).  `targets`: general regime, equal NaN / +inf /
    -inf classes and |kernel - ref64| <= 2 * C_ENC_MEASURED * 2^-24 * scale elsewhere;
  * dib_box_decode -- exact regime: dw = dh = 0, weights 1, integer anchors and dx in halves: every operation is exact,
    bit for bit, NaN deltas at equal positions, R = 1 / 255 / 256 / 257 and R = 3 A (the r % A reuse).  General regime:
    2 * C_DEC_MEASURED * 2^-24 * scale, both weight sets, deltas beyond the clip;
  * dib_box_pool, dib_box_labels -- exact (integer / copy semantics): P 0 / 1 / 300, Gpad 0 / G / G + 3, `ok` absent and
    present, M across 256, match values -2, -1 and indices;
  * dib_det_candidates -- general regime: C 2 / 3 / 64 / 65 / 91 / 127 / 128, R 1 / 3 / 4 / 5 / 257, logit spreads 1.5
    and 4, a saturated row (and one whose other scores underflow), a NaN-box class, two image shapes.  Outside `near`
    the kept mask equals the reference's; kept scores within 2 * C_SM_MEASURED * 2^-24 * sscale, boxes within the decode
    bound; a `near` candidate is either dropped (-inf) or kept within the same bounds; stats[0] = the number of finite
    scores written, stats[1] = bit for bit the largest coordinate among the kernel's kept boxes.

Edge cases constructed in the exact regime (the CPU half asserts that each occurs): IoU exactly 1/2, 7/10, 3/10 (and
1/20, 1/100 for the third threshold pair), IoU one integer step below 1/2, 7/10 and 3/10 (5000, 7000, 3000 over 10001),
duplicate ground truths, a candidate equal to a ground truth, a zero-area candidate on a zero-area ground truth (0 / 0),
a zero-area candidate inside a real ground truth, a ground truth that overlaps no candidate (its best IoU is 0: the
low-quality restore reaches every candidate with IoU 0), a ground truth whose best is attained by candidates in
different waves and in different 256-blocks, reversed candidates (x2 < x1: a positive union, a negative one that gives
-0, and a zero one that gives NaN).

The constants C_*_MEASURED are MEASUREMENTS of the plain float32 torch path on the CPU (BoxCoder.encode / decode,
torch.softmax) against the float64 references over the cases of this file, never of a HIP kernel; the CPU half prints
and asserts them.  The kernels get 2 x: they do the same operations in the same order, and only the device's logf /
expf / divide may be about an ulp looser than the CPU's."""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import dib_oracle as O
from detectinblur_amd.models import detector_ops as ops

U = 2.0 ** -24                  # fp32 unit roundoff
# The distance between two IoUs (or an IoU and a threshold) below which float32 may decide the other way.  With u = 2^-24
# and every operation rounded once: each area (two differences, one product) and the intersection (two differences --
# the min / max are exact --, one product) carry 3 roundings; the union a + b - inter carries 2 more on terms that are
# each <= the union (inter <= min(a, b), so the union >= max(a, b)): (3 + 3 + 3 + 2 * 2) u ~ 15 u with the partial sum
# a + b <= 2 union counted twice; the quotient carries 1 and inherits the numerator's 3: <= ~19 u relative on an IoU
# <= 1, rounded up to 32 u.  test_general_match_iou_error_and_near_cap asserts it on the float32 torch path.
GUARD = 32 * U
NEAR_CAP = 0.01                 # at most this fraction of a case's candidates (det: class candidates) may be `near`

# Largest |float32 torch path on the CPU - float64 reference| / (2^-24 * scale) over the cases of this file, rounded up in
# the third digit: test_torch_paths_are_within_the_bounds_and_measure_c prints and asserts them.
C_ENC_MEASURED, C_DEC_MEASURED, C_SM_MEASURED, C_MARGIN = 2.97, 2.83, 5.03, 2.0
C_ENC, C_DEC, C_SM = C_ENC_MEASURED * C_MARGIN, C_DEC_MEASURED * C_MARGIN, C_SM_MEASURED * C_MARGIN

THRESHOLDS = ((0.7, 0.3), (0.5, 0.5), (0.05, 0.01))
WEIGHTS = ((1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0))
CLIP = O.DECODE_CLIP


# ------------------------------------------------------------------------------------------------------- exact regime

EXACT_CASES = OrderedDict([            # name -> (ground truths per image, M, candidates shared by the images)
    ("n5_shared_m1023", ([256, 0, 1, 255, 2], 1023, True)),
    ("n5_per_m257", ([2, 255, 0, 256, 1], 257, False)),
    ("n32_shared_m64", ([(7 * i) % 13 for i in range(32)], 64, True)),
    ("n1_per_m1", ([2], 1, False)),
    ("n1_shared_m63", ([1], 63, True)),
    ("n5_per_m255", ([1, 2, 0, 40, 256], 255, False)),
    ("n1_shared_m256", ([255], 256, True)),
])

STRIP_Y = 884                   # random boxes end at y = 880; the constructed pairs live below, 110 columns apart
# name, (num, den) of the IoU, ground truth (w, h), candidate (w, h) in the ground truth's corner: IoU = wh / WH
PAIRS = [("1/2", (1, 2), (100, 100), (50, 100)), ("1/2-", (5000, 10001), (73, 137), (50, 100)),
         ("7/10", (7, 10), (100, 100), (70, 100)), ("7/10-", (7000, 10001), (73, 137), (70, 100)),
         ("3/10", (3, 10), (100, 100), (30, 100)), ("3/10-", (3000, 10001), (73, 137), (30, 100)),
         ("1/20", (1, 20), (40, 25), (10, 5)), ("1/100", (1, 100), (40, 25), (5, 2))]
PAIR_CAND0 = 10                 # candidate slot of the first pair
REAL_GT = [100, 100, 160, 180]
ISOLATED_GT = [1000, 884, 1020, 900]
POINT = [950, 950, 950, 950]


def _int_boxes(rs, n):
    """Random integer boxes inside [0, 1024) x [0, 880], half of them on an 8-pixel grid (equal IoUs of unequal boxes)."""
    x1, y1 = rs.randint(0, 1000, n), rs.randint(0, 860, n)
    w, h = rs.randint(1, 201, n), rs.randint(1, 201, n)
    grid = rs.rand(n) < 0.5
    for a in (x1, y1, w, h):
        a[grid] = (a[grid] + 7) // 8 * 8
    return np.stack([x1, y1, np.minimum(x1 + w, 1023), np.minimum(y1 + h, 880)], 1).astype(np.int64)


def _place(gt, cand):
    """Write the constructed rows into one image's ground truth [G, 4] and its candidates [M, 4], as far as they fit."""
    G, M = len(gt), len(cand)
    if G >= 8 and M >= PAIR_CAND0 + 8:
        for k, (_, _, (W, H), (w, h)) in enumerate(PAIRS):
            gt[G - 8 + k] = [110 * k, STRIP_Y, 110 * k + W, STRIP_Y + H]
            cand[PAIR_CAND0 + k] = [110 * k, STRIP_Y, 110 * k + w, STRIP_Y + h]
    if G >= 16 and M >= 255:
        gt[0] = REAL_GT
        gt[G - 9] = ISOLATED_GT
        gt[G - 10] = POINT
        gt[G - 11] = gt[1]                                             # duplicates: the lower index wins
        cand[20] = gt[1]                                               # IoU 1 with both
        cand[21] = POINT                                               # 0 / 0
        cand[22] = [120, 120, 120, 150]                                # zero area inside REAL_GT
        cand[23] = [150, 110, 110, 170]                                # reversed, union with REAL_GT 2400
        cand[24] = [400, 100, 100, 400]                                # reversed, every union negative: IoU -0
        cand[25] = [160, 100, 100, 180]                                # reversed, area -4800: 0 / 0 with REAL_GT
        for j in (5, 70, 700 if M > 700 else M - 1):                   # the best of "7/10-" in three waves / two blocks
            cand[j] = cand[PAIR_CAND0 + 3]


@functools.lru_cache(maxsize=None)
def _exact_case(name):
    counts, M, shared = EXACT_CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    gts = [_int_boxes(rs, g) for g in counts]
    cand = _int_boxes(rs, M) if shared else np.stack([_int_boxes(rs, M) for _ in counts])
    for n, gt in enumerate(gts):
        c = cand if shared else cand[n]
        take = rs.randint(0, M, max(M // 16, 1))                       # candidates that are copies of other candidates
        c[take] = c[rs.randint(0, M, take.size)]
        if len(gt):
            hit = rs.randint(0, M, max(M // 32, 1))                    # and of ground truths
            c[hit] = gt[rs.randint(0, len(gt), hit.size)]
    for n, gt in enumerate(gts):
        _place(gt, cand if shared else cand[n])
    return dict(gts=gts, cand=cand, shared=shared, M=M)


def _image_cands(case, n):
    return case["cand"] if case["shared"] else case["cand"][n]


def _int_iou(gt, cand):
    """inter, union [G, M] int64 and the two area vectors."""
    a, b = gt[:, None, :], cand[None, :, :]
    w = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), 0)
    h = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), 0)
    area = lambda x: (x[:, 2] - x[:, 0]) * (x[:, 3] - x[:, 1])
    inter = w * h
    return inter, area(gt)[:, None] + area(cand)[None, :] - inter, area(gt), area(cand)


def _exact_want(case, high, low, allow):
    return np.stack([O.match64(g, _image_cands(case, n), high, low, allow) for n, g in enumerate(case["gts"])])


def _decode_exact_case(R, A, seed):
    """Integer anchors, deltas (dx, dy, 0, 0) with dx in halves, a few NaN entries: every float32 operation of
    BoxCoder.decode with weights 1 is exact (products and sums of half-integers below 2^12, exp(0) = 1)."""
    rs = np.random.RandomState(seed)
    anchors = _int_boxes(rs, A).astype(np.float32)
    deltas = np.zeros((R, 4), dtype=np.float32)
    deltas[:, :2] = rs.randint(-4, 5, (R, 2)) / 2.0
    nan = rs.rand(R, 4) < 0.05
    nan[0, 2] = True
    deltas[nan] = np.nan
    return deltas, anchors


DECODE_EXACT = [(1, 1), (255, 85), (256, 256), (257, 257), (768, 256), (771, 257)]


def _pool_cases():
    """(counts, P, Gpad, ok present)"""
    return [([0, 0, 0], 1, 0, False), ([4, 0, 9, 1], 0, 9, False), ([4, 0, 9, 1], 1, 9, True), ([4, 0, 9, 1], 300, 12, True),
            ([256, 3], 1, 259, False), ([5, 256, 0], 300, 256, True), ([0, 0], 300, 0, True), ([7], 255, 8, False)]


def _pool_inputs(counts, P, Gpad, with_ok, seed):
    rs = np.random.RandomState(seed)
    gts = [_int_boxes(rs, g).astype(np.float32) + np.float32(0.25) for g in counts]
    props = np.stack([_int_boxes(rs, P).astype(np.float32) for _ in counts]).reshape(len(counts), P, 4)
    labels = [rs.randint(1, 91, g).astype(np.int64) for g in counts]
    M = P + Gpad
    match = np.stack([rs.randint(-2, max(g, 1), M) for g in counts]).astype(np.int64)
    match[:, ::7] = -2
    match[:, 1::7] = -1
    ok = (rs.rand(len(counts), P) < 0.8) if with_ok else None
    return gts, props, labels, match, ok


# ----------------------------------------------------------------------------------------------------- general regime

def _rand_boxes(rs, n, W, H, degenerate=0.0):
    """The draw of tests/test_detect_fuzz_gpu.py in float32: corners anywhere, sides rand^2 * half the canvas, a share of
    zero-area boxes."""
    xy = (rs.rand(n, 2).astype(np.float32) * np.array([W, H], dtype=np.float32))
    wh = (rs.rand(n, 2).astype(np.float32) ** 2 * np.array([W / 2.0, H / 2.0], dtype=np.float32))
    if degenerate:
        wh[rs.rand(n) < degenerate] = 0.0
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


GENERAL_CASES = OrderedDict([          # name -> (seed, ground truths per image, M, shared, gt degenerate share, duplicates)
    ("n3_shared_m600_deg", (0, [40, 0, 17], 600, True, 0.1, True)),
    ("n4_per_m257", (1, [1, 40, 23, 5], 257, False, 0.0, False)),
    ("n1_shared_m64_deg", (2, [9], 64, True, 0.1, True)),
    ("n2_per_m511_dup", (3, [31, 40], 511, False, 0.0, True)),
    ("n4_shared_m600", (4, [12, 2, 40, 0], 600, True, 0.0, False)),
    ("n2_per_m300_deg", (5, [40, 8], 300, False, 0.1, False)),
])
CANVAS = (1333.0, 800.0)


@functools.lru_cache(maxsize=None)
def _general_case(name):
    seed, counts, M, shared, deg, dup = GENERAL_CASES[name]
    rs = np.random.RandomState(500 + seed)
    gts = [_rand_boxes(rs, g, *CANVAS, degenerate=deg) for g in counts]
    for g in gts:
        if dup and len(g) > 3:
            g[len(g) - 1] = g[0]
    cand = _rand_boxes(rs, M, *CANVAS, degenerate=0.05) if shared else np.stack([_rand_boxes(rs, M, *CANVAS, degenerate=0.05) for _ in counts])
    for n, g in enumerate(gts):                                        # exact hits
        if len(g) and M > 2:
            (cand if shared else cand[n])[1 + (n if shared else 0)] = g[0]
    match = np.stack([rs.randint(-2, max(len(g), 1), M) for g in gts]).astype(np.int64)
    deltas = (rs.randn(len(counts) * M, 4) * [0.5, 0.5, 3.0, 3.0]).astype(np.float32)
    deltas[5 % len(deltas)] = np.nan
    deltas[6 % len(deltas), 2] = 50.0
    deltas[7 % len(deltas), 3] = -50.0
    deltas[8 % len(deltas), 0] = np.nan
    return dict(gts=gts, cand=cand, shared=shared, M=M, match=match, deltas=deltas)


def _matched_ref(case, n):
    """gt[match.clamp(min = 0)] of image n, a zero box for an image without ground truth."""
    g = case["gts"][n]
    return g[np.maximum(case["match"][n], 0)] if len(g) else np.zeros((case["M"], 4), dtype=np.float32)


def _check_accept(got, accept, what):
    got = np.asarray(got, dtype=np.int64)
    assert got.min() >= -2 and got.max() < accept.shape[1] - 2, (what, int(got.min()), int(got.max()))
    bad = ~accept[np.arange(len(got)), got + 2]
    assert not bad.any(), "%s: %d answers outside the acceptable set, first at %s: %s" % (
        what, int(bad.sum()), np.flatnonzero(bad)[:4].tolist(), got[bad][:4].tolist())


def _check_close(got, ref, scale, c, what):
    """Equal NaN, +inf and -inf classes; elsewhere |got - ref| <= c * 2^-24 * scale.  Returns the largest ratio / c."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    for name, f in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        bad = f(got) != f(ref)
        assert not bad.any(), "%s: %d elements differ in the %s class, first at %s" % (what, int(bad.sum()), name, np.argwhere(bad)[:4].tolist())
    fin = np.isfinite(ref)
    d, bound = np.abs(got[fin] - ref[fin]), c * U * scale[fin]
    assert np.isfinite(bound).all(), what
    bad = d > bound
    assert not bad.any(), "%s: %d elements outside their bound, worst |d| / bound %.3g" % (
        what, int(bad.sum()), float((d[bad] / np.maximum(bound[bad], 1e-300)).max()))
    return float((d / np.maximum(bound, 1e-300)).max()) if d.size else 0.0


DET_CASES = OrderedDict([              # name -> (C, R, logit spread, image shape, weights)
    ("c2_r257", (2, 257, 1.5, (800, 1333), WEIGHTS[1])),
    ("c3_r1", (3, 1, 4.0, (480, 640), WEIGHTS[1])),
    ("c64_r3", (64, 3, 1.5, (800, 1333), WEIGHTS[1])),
    ("c65_r4", (65, 4, 4.0, (480, 640), WEIGHTS[0])),
    ("c91_r5", (91, 5, 1.5, (800, 1333), WEIGHTS[1])),
    ("c127_r257", (127, 257, 4.0, (480, 640), WEIGHTS[1])),
    ("c128_r257", (128, 257, 1.5, (800, 1333), WEIGHTS[1])),
    ("c91_r257", (91, 257, 4.0, (800, 1333), WEIGHTS[0])),
])
SCORE_THRESH, MIN_SIZE = 0.05, 1e-2


@functools.lru_cache(maxsize=None)
def _det_case(name):
    C, R, spread, shape, weights = DET_CASES[name]
    rs = np.random.RandomState(700 + C + R)
    logits = (rs.randn(R, C) * spread).astype(np.float32)
    deltas = (rs.randn(R, C, 4) * [1.0, 1.0, 2.0, 2.0] * (np.array(weights) / [10.0, 10.0, 5.0, 5.0]) * [1, 1, 2.5, 2.5]).astype(np.float32)
    rois = _rand_boxes(rs, R, shape[1], shape[0], degenerate=0.05)
    rois = np.minimum(rois, np.array([shape[1], shape[0]] * 2, dtype=np.float32))
    rois[0] = [100.3, 50.7, 300.9, 260.1]                              # the saturated row's RoI is a real box
    logits[0, 1] = 30.0                                                # a saturated row
    if R > 2:
        logits[2, C - 1] = 100.0                                       # and one whose other scores underflow in float32
        deltas[1, C - 1] = np.nan                                      # a NaN box: dropped
        deltas[2, 1, 2] = 50.0 * weights[2]                            # beyond the clip
    ref = O.det_candidates64(logits, deltas.reshape(R, 4 * C), rois, shape, weights, CLIP, SCORE_THRESH, MIN_SIZE, c_score=C_SM, c_box=C_DEC)
    return dict(logits=logits, deltas=deltas.reshape(R, 4 * C), rois=rois, shape=shape, weights=weights, ref=ref)


def _check_det(ref, scores, boxes, stats, what):
    """scores [C - 1, R] float32 (-inf = dropped), boxes [C - 1, R, 4], stats (count, bits of the largest coordinate) or
    None against det_candidates64's result.  Returns (score ratio / c, box ratio / c)."""
    scores, boxes = np.asarray(scores), np.asarray(boxes)
    fin = np.isfinite(scores)
    assert (fin | np.isneginf(scores)).all(), "%s: a score is NaN or +inf" % what
    rb = _check_close(boxes, ref["boxes"], ref["bscale"], C_DEC, what + " boxes")
    clear = ~ref["near"]
    bad = (fin != ref["kept"]) & clear
    assert not bad.any(), "%s: %d candidates kept / dropped against the reference away from every threshold, first at %s" % (
        what, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    d, bound = np.abs(scores[fin].astype(np.float64) - ref["scores"][fin]), C_SM * U * ref["sscale"][fin]
    assert (d <= bound).all(), "%s: %d kept scores outside their bound, worst |d| / bound %.3g" % (what, int((d > bound).sum()), float((d / bound).max()))
    if stats is not None:
        assert int(stats[0]) == int(fin.sum()), (what, int(stats[0]), int(fin.sum()))
        big = boxes[fin].max() if fin.any() else np.float32(0)
        assert int(stats[1]) == int(np.array([big], dtype=np.float32).view(np.uint32)[0]), (what, int(stats[1]), float(big))
    return (float((d / bound).max()) if d.size else 0.0), rb


def _torch_det(case):
    """The plain float32 torch path on the CPU in the kernel's output form."""
    coder = ops.BoxCoder(case["weights"], clip=CLIP)
    s = torch.softmax(torch.tensor(case["logits"]), -1)[:, 1:].t()
    b = ops.clip_boxes_to_image(coder.decode(torch.tensor(case["deltas"]), torch.tensor(case["rois"])), case["shape"])[:, 1:].permute(1, 0, 2)
    ok = (s > SCORE_THRESH) & ((b[..., 2] - b[..., 0]) >= MIN_SIZE) & ((b[..., 3] - b[..., 1]) >= MIN_SIZE)
    s, b, ok = s.numpy(), b.contiguous().numpy(), ok.numpy()
    big = b[ok].max() if ok.any() else np.float32(0)
    return np.where(ok, s, -np.inf).astype(np.float32), b, (int(ok.sum()), int(np.array([big], dtype=np.float32).view(np.uint32)[0]))


# ================================================================================================================ CPU

def _t64(a):
    return torch.tensor(np.asarray(a, dtype=np.float64).reshape(-1, 4))


def _torch_match(gt, cand, high, low, allow, dtype):
    if len(gt) == 0:
        return np.full(len(cand), -1, dtype=np.int64)
    q = ops.box_iou(_t64(gt).to(dtype), _t64(cand).to(dtype))
    return ops.Matcher(high, low, allow)(q).numpy()


def test_hand_computed_three_box_cases():
    gt = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [20, 20, 30, 30]])
    cand = np.array([[0, 0, 5, 10], [21, 21, 29, 29], [50, 50, 60, 60]])
    q = O.box_iou64(gt, cand)
    assert q.tolist() == [[0.5, 0.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.64, 0.0]]
    assert O.match64(gt, cand, 0.7, 0.3, False).tolist() == [-2, -2, -1]           # 0.5 and 0.64 between, 0 below
    assert O.match64(gt, cand, 0.7, 0.3, True).tolist() == [0, 2, -1]              # each best restored, the lower duplicate
    assert O.match64(gt, cand, 0.5, 0.5, False).tolist() == [0, 2, -1]             # 0.5 >= 0.5
    assert O.match64(gt, cand, 0.64, 0.5, False).tolist() == [-2, 2, -1]           # float32(16 / 25) >= float32(0.64)
    assert O.match64(gt[:0], cand, 0.7, 0.3, True).tolist() == [-1, -1, -1]
    # a ground truth that overlaps nothing: its best is 0, and every candidate with IoU 0 to it goes back to its argmax
    lonely = np.array([[0, 0, 10, 10], [100, 100, 110, 110]])
    assert O.match64(lonely, cand, 0.7, 0.3, True).tolist() == [0, 0, 0]
    assert O.match64(lonely, cand, 0.7, 0.3, False).tolist() == [-2, -1, -1]
    # 0 / 0: NaN wins the candidate's maximum (index 1 here), and the ground truth's best is NaN, which restores nothing
    pt = np.array([[0, 0, 10, 10], [5, 5, 5, 5], [20, 20, 30, 30]])
    cp = np.array([[5, 5, 5, 5], [0, 0, 10, 10], [21, 21, 29, 29]])
    assert np.isnan(O.box_iou64(pt, cp)[1, 0])
    assert O.match64(pt, cp, 0.7, 0.3, False).tolist() == [1, 0, -2]
    assert O.match64(pt, cp, 0.7, 0.3, True).tolist() == [1, 0, 2]
    # reversed candidate: area -100, inter 0, union 100 - 100 = 0 -> NaN; area -400 -> 0 / -300 = -0 -> below
    rv = np.array([[10, 0, 0, 10], [20, 0, 0, 20]])
    assert O.match64(pt[:1], rv, 0.7, 0.3, False).tolist() == [0, -1]
    # guard: 0.5 against the threshold 0.5 is near (either class), 0.64 against 0.7 / 0.3 is not
    m, acc, near = O.match64(gt, cand, 0.5, 0.5, False, guard=GUARD)
    assert m.tolist() == [0, 2, -1] and near.tolist() == [True, False, False]
    assert acc[0].tolist() == [False, True, True, False, False] and acc[1].tolist() == [False, False, False, False, True]
    m, acc, near = O.match64(gt, cand, 0.7, 0.3, True, guard=GUARD)
    assert not near.any() and acc.sum() == 3 and acc[0, 2] and acc[1, 4] and acc[2, 1]
    # two different ground truths within the guard of each other: either index, near
    close = np.array([[0, 0, 10, 10], [0, 0, 10, 10.000001]], dtype=np.float32)
    m, acc, near = O.match64(close, np.array([[0, 0, 10, 9]]), 0.7, 0.3, False, guard=GUARD)
    assert near.tolist() == [True] and acc[0].tolist() == [False, False, True, True]
    # encode / decode by hand: reference box (2, 4, 6, 12) against (0, 0, 4, 4): centres (4, 8) and (2, 2)
    t, sc = O.box_encode64([[2, 4, 6, 12]], [[0, 0, 4, 4]], (10, 10, 5, 5))
    assert np.allclose(t, [[10 * 2 / 4.0, 10 * 6 / 4.0, 5 * np.log(1.0), 5 * np.log(2.0)]], rtol=1e-15)
    assert np.allclose(sc, [[10 * 6 / 4.0, 10 * 10 / 4.0, 5.0, 5 * (1 + np.log(2.0))]], rtol=1e-15)
    b, sc = O.box_decode64(np.float32(t), [[0, 0, 4, 4]], (10, 10, 5, 5))
    assert np.allclose(b, [[2, 4, 6, 12]], atol=1e-6)
    b, _ = O.box_decode64([[0, 0, 50, -1]], [[0, 0, 4, 4]], (1, 1, 1, 1))
    assert np.allclose(b[0, [0, 2]], [2 - 2 * 62.5, 2 + 2 * 62.5], rtol=1e-6) and np.allclose(b[0, [1, 3]], [2 - 2 / np.e, 2 + 2 / np.e])


@pytest.mark.parametrize("name", list(EXACT_CASES))
def test_exact_cases_meet_the_exactness_condition_and_pin_match64(name):
    """The inputs are integers in [0, 1024) with every area, intersection and union below 2^24 in magnitude; on them
    match64(guard = 0) equals torch's Matcher on box_iou in float64 AND in float32 (the CPU's float32 IoU is the one
    correctly rounded quotient as well)."""
    case = _exact_case(name)
    for n, gt in enumerate(case["gts"]):
        c = _image_cands(case, n)
        for a in (gt, c):
            assert a.dtype == np.int64 and (a >= 0).all() and (a < 1024).all()
        inter, union, ag, ac = _int_iou(gt, c)
        assert max(np.abs(inter).max(initial=0), np.abs(union).max(initial=0), np.abs(ag).max(initial=0), np.abs(ac).max(initial=0)) < 2 ** 24
        q = O.box_iou64(gt, c)
        ok = union != 0
        assert np.array_equal(q[ok], inter[ok] / union[ok]) and np.isnan(q[~ok & (inter == 0)]).all()
        for (high, low) in THRESHOLDS:
            for allow in (False, True):
                want = O.match64(gt, c, high, low, allow)
                for dtype in (torch.float64, torch.float32):
                    got = _torch_match(gt, c, high, low, allow, dtype)
                    assert np.array_equal(got, want), (name, n, high, low, allow, dtype, np.flatnonzero(got != want)[:4].tolist())


def test_exact_cases_contain_every_constructed_row():
    n = dict.fromkeys([p[0] for p in PAIRS] + ["dup_gt", "cand_is_gt", "0/0", "zero_in_gt", "lonely_gt", "best_in_blocks", "best_in_waves",
                                               "reversed", "reversed_-0", "reversed_nan", "G", "M", "N", "restore_all"], 0)
    seen_g, seen_m, seen_n, values = set(), set(), set(), set()
    for name in EXACT_CASES:
        case = _exact_case(name)
        seen_m.add(case["M"]); seen_n.add(len(case["gts"]))
        for i, gt in enumerate(case["gts"]):
            seen_g.add(len(gt))
            if not len(gt):
                continue
            c = _image_cands(case, i)
            inter, union, ag, ac = _int_iou(gt, c)
            q = O.box_iou64(gt, c)
            _, arg = O._max_first(q, 0)
            cols = np.arange(len(c))
            for pname, (num, den), _, _ in PAIRS:
                hit = (inter[arg, cols] * den == num * union[arg, cols]) & (union[arg, cols] > 0) & (inter[arg, cols] > 0)
                if num > 1000:
                    hit &= union[arg, cols] == den
                n[pname] += int(hit.sum())
            same = (gt[:, None] == gt[None]).all(-1)
            n["dup_gt"] += int(np.triu(same, 1).any())
            n["cand_is_gt"] += int(((gt[:, None] == c[None]).all(-1) & (ag > 0)[:, None]).any())
            n["0/0"] += int(((ag == 0)[:, None] & (ac == 0)[None] & np.isnan(q)).any())
            inside = (c[None, :, 0] > gt[:, None, 0]) & (c[None, :, 2] < gt[:, None, 2]) & (c[None, :, 1] > gt[:, None, 1]) & (c[None, :, 3] < gt[:, None, 3])
            n["zero_in_gt"] += int((inside & (ac == 0)[None] & (ag > 0)[:, None]).any())
            lonely = (inter == 0).all(axis=1) & (ag > 0)
            n["lonely_gt"] += int(lonely.any())
            if lonely.any():                                           # ... and then the restore reaches every candidate with IoU 0 to it
                m = O.match64(gt, c, 0.7, 0.3, True)
                n["restore_all"] += int((m[(q[np.flatnonzero(lonely)[0]] == 0)] >= 0).all() and (O.match64(gt, c, 0.7, 0.3, False) < 0).any())
            best, _ = O._max_first(q, 1)
            for g in np.flatnonzero(best > 0):
                idx = np.flatnonzero(q[g] == best[g])
                n["best_in_blocks"] += int(len(set(idx // 256)) > 1)
                n["best_in_waves"] += int(any(len(set(idx[idx // 256 == b] // 64)) > 1 for b in set(idx // 256)))
            rev = c[:, 2] < c[:, 0]
            n["reversed"] += int(rev.sum())
            n["reversed_-0"] += int((rev[None] & (q == 0) & np.signbit(q)).any())
            n["reversed_nan"] += int((rev[None] & np.isnan(q)).any())
            for (high, low) in THRESHOLDS:
                for allow in (False, True):
                    values |= set(np.unique(O.match64(gt, c, high, low, allow)).tolist())
    n["G"], n["M"], n["N"] = int(seen_g >= {0, 1, 2, 255, 256}), int(seen_m >= {1, 63, 64, 255, 256, 257, 1023}), int(seen_n >= {1, 5, 32})
    print(sorted(n.items()))
    assert all(v > 0 for v in n.values()), sorted(n.items())
    assert {-2, -1, 0, 255} <= values


def test_references_equal_the_float64_torch_path():
    """box_encode64 / box_decode64 / det_candidates64 against BoxCoder and softmax run in float64 (decode: torch divides
    by the weights in float64, as the reference does)."""
    for name in GENERAL_CASES:
        case = _general_case(name)
        for weights in WEIGHTS:
            coder = ops.BoxCoder(weights, clip=CLIP)
            for n in range(len(case["gts"])):
                c = _image_cands(case, n)
                t, _ = O.box_encode64(_matched_ref(case, n), c, weights)
                want = coder.encode(_t64(_matched_ref(case, n)), _t64(c)).numpy()
                assert np.allclose(t, want, rtol=1e-12, atol=0, equal_nan=True), (name, n)
            if case["shared"]:
                d = case["deltas"] * np.array(weights, dtype=np.float32)
                b, sc = O.box_decode64(d, case["cand"], weights)
                want = coder.decode(_t64(d), torch.cat([_t64(case["cand"])] * len(case["gts"]))).reshape(-1, 4).numpy()
                assert np.allclose(b, want, rtol=1e-12, atol=1e-9, equal_nan=True), name
                assert (np.abs(b) <= sc * (1 + 1e-12))[np.isfinite(b)].all()
    for name in DET_CASES:
        case = _det_case(name)
        ref = case["ref"]
        coder = ops.BoxCoder(case["weights"], clip=CLIP)
        s = torch.softmax(torch.tensor(case["logits"]).double(), -1)[:, 1:].t().numpy()
        b = ops.clip_boxes_to_image(coder.decode(torch.tensor(case["deltas"]).double(), torch.tensor(case["rois"]).double()), case["shape"])
        b = b[:, 1:].permute(1, 0, 2).numpy()
        assert np.allclose(ref["scores"], s, rtol=1e-12, atol=1e-300) and np.allclose(ref["boxes"], b, rtol=1e-12, atol=1e-9, equal_nan=True)
        assert ref["kept"][0, 0] and ref["kept"].sum() > 0, name


def test_general_match_iou_error_and_near_cap():
    """On every general case: the float32 torch IoU stays within the guard of box_iou64; at most 1 % of the candidates
    are `near`; the float32 torch Matcher's answers lie in the acceptable sets."""
    worst, most = 0.0, 0.0
    for name in GENERAL_CASES:
        case = _general_case(name)
        for (high, low) in THRESHOLDS:
            for allow in (False, True):
                n_near = 0
                for n, gt in enumerate(case["gts"]):
                    c = _image_cands(case, n)
                    m, acc, near = O.match64(gt, c, high, low, allow, guard=GUARD)
                    n_near += int(near.sum())
                    _check_accept(_torch_match(gt, c, high, low, allow, torch.float32), acc, "%s image %d torch" % (name, n))
                    _check_accept(m, acc, "%s image %d ref" % (name, n))
                    assert (acc.sum(axis=1) == 1)[~near].all()
                frac = n_near / float(len(case["gts"]) * case["M"])
                most = max(most, frac)
                assert frac <= NEAR_CAP, (name, high, low, allow, frac)
        for n, gt in enumerate(case["gts"]):
            if len(gt):
                c = _image_cands(case, n)
                q32 = ops.box_iou(torch.tensor(gt), torch.tensor(c)).numpy().astype(np.float64)
                q = O.box_iou64(gt, c)
                assert np.array_equal(np.isnan(q32), np.isnan(q)), (name, n)
                worst = max(worst, float(np.nanmax(np.abs(q32 - q), initial=0.0)))
    print("largest float32 IoU error %.2f u, largest near share %.4f" % (worst / U, most))
    assert worst <= GUARD


def test_torch_paths_are_within_the_bounds_and_measure_c():
    """BoxCoder.encode / decode and torch.softmax in float32 on the CPU against the float64 references over the cases the
    GPU half uses: within the bounds the kernels are held to, and the largest ratios are what C_*_MEASURED quote."""
    enc = dec = sm = dbox = 0.0
    for name in GENERAL_CASES:
        case = _general_case(name)
        for weights in WEIGHTS:
            coder = ops.BoxCoder(weights, clip=CLIP)
            for n in range(len(case["gts"])):
                c, r = _image_cands(case, n), _matched_ref(case, n)
                t, sc = O.box_encode64(r, c, weights)
                got = coder.encode(torch.tensor(r), torch.tensor(c)).numpy()
                enc = max(enc, C_ENC * _check_close(got, t, sc, C_ENC, "%s torch encode" % name))
            if case["shared"]:
                d = case["deltas"] * np.array(weights, dtype=np.float32)
                b, sc = O.box_decode64(d, case["cand"], weights)
                got = coder.decode(torch.tensor(d), torch.cat([torch.tensor(case["cand"])] * len(case["gts"]))).reshape(-1, 4).numpy()
                dec = max(dec, C_DEC * _check_close(got, b, sc, C_DEC, "%s torch decode" % name))
    for name in DET_CASES:
        case = _det_case(name)
        s, b, stats = _torch_det(case)
        assert case["ref"]["near"].mean() <= NEAR_CAP, (name, case["ref"]["near"].mean())
        rs_, rb_ = _check_det(case["ref"], s, b, stats, name + " torch")
        s32 = torch.softmax(torch.tensor(case["logits"]), -1)[:, 1:].t().numpy().astype(np.float64)
        sm = max(sm, float((np.abs(s32 - case["ref"]["scores"]) / (U * case["ref"]["sscale"])).max()))
        dbox = max(dbox, C_DEC * rb_)
        print("%-12s softmax ratio %.3f  box ratio %.3f  near %d  kept %d" % (name, sm, C_DEC * rb_, int(case["ref"]["near"].sum()), int(case["ref"]["kept"].sum())))
    print("measured constants: encode %.3f, decode %.3f (detections' boxes %.3f), softmax %.3f" % (enc, dec, dbox, sm))
    assert enc <= C_ENC_MEASURED and max(dec, dbox) <= C_DEC_MEASURED and sm <= C_SM_MEASURED, (enc, dec, dbox, sm)


def test_near_candidates_cannot_hide_garbage():
    """A score threshold set ON a candidate's score makes it `near`: the check accepts the candidate kept with the right
    score or dropped, and nothing else; a candidate away from every threshold cannot change sides."""
    case = dict(_det_case("c91_r5"))
    ref0 = case["ref"]
    k = np.argwhere(ref0["kept"] & (ref0["scores"] == ref0["scores"][ref0["kept"]].min()))[0]       # the lowest kept score
    thr = float(np.float32(ref0["scores"][tuple(k)]))
    ref = O.det_candidates64(case["logits"], case["deltas"], case["rois"], case["shape"], case["weights"], CLIP, thr, MIN_SIZE, c_score=C_SM, c_box=C_DEC)
    assert ref["near"][tuple(k)] and ref["near"].sum() <= 2, np.argwhere(ref["near"]).tolist()
    s = np.where(ref["kept"], ref["scores"], -np.inf).astype(np.float32)
    b = ref["boxes"].astype(np.float32)
    for v in (np.float32(ref["scores"][tuple(k)]), np.float32(-np.inf)):
        t = s.copy(); t[tuple(k)] = v
        _check_det(ref, t, b, None, "near")
    for v in (np.float32(thr * 1.01), np.float32(thr + 0.01), np.float32(0.0), np.float32(np.nan), np.float32(np.inf)):
        t = s.copy(); t[tuple(k)] = v
        with pytest.raises(AssertionError):
            _check_det(ref, t, b, None, "near")
    other = np.argwhere(ref["kept"] & ~ref["near"])[0]
    t = s.copy(); t[tuple(other)] = -np.inf
    with pytest.raises(AssertionError):
        _check_det(ref, t, b, None, "clear")
    lost = np.argwhere(~ref["kept"] & ~ref["near"])[0]
    t = s.copy(); t[tuple(lost)] = np.float32(ref["scores"][tuple(lost)])
    with pytest.raises(AssertionError):
        _check_det(ref, t, b, None, "clear")
    bb = b.copy(); bb[tuple(other)] += 0.01
    with pytest.raises(AssertionError):
        _check_det(ref, s, bb, None, "box")
    # stats: a wrong count and a wrong largest coordinate are caught
    fin = np.isfinite(s)
    bits = int(np.array([b[fin].max()], dtype=np.float32).view(np.uint32)[0])
    _check_det(ref, s, b, (int(fin.sum()), bits), "stats")
    for stats in ((int(fin.sum()) + 1, bits), (int(fin.sum()), bits + 1)):
        with pytest.raises(AssertionError):
            _check_det(ref, s, b, stats, "stats")
    # and a match outside the acceptable set
    gt, cand = np.array([[0, 0, 10, 10], [20, 20, 30, 30]]), np.array([[0, 0, 5, 10], [50, 50, 60, 60]])
    m, acc, near = O.match64(gt, cand, 0.5, 0.5, False, guard=GUARD)
    assert near.tolist() == [True, False]
    _check_accept([0, -1], acc, "x"); _check_accept([-1, -1], acc, "x")
    for wrong in ([1, -1], [-2, -1], [0, 0], [0, -2]):
        with pytest.raises(AssertionError):
            _check_accept(wrong, acc, "x")


def test_pool64_and_labels64_by_hand():
    gts = [np.array([[1, 2, 3, 4]], dtype=np.float32), np.zeros((0, 4), dtype=np.float32)]
    props = np.arange(16, dtype=np.float32).reshape(2, 2, 4)
    out = O.pool64(props, gts, 2)
    assert out.tolist() == [[[0, 1, 2, 3], [4, 5, 6, 7], [1, 2, 3, 4], [0, 0, 1, 1]], [[8, 9, 10, 11], [12, 13, 14, 15], [0, 0, 1, 1], [0, 0, 1, 1]]]
    match = np.array([[0, -1, -2, 0], [0, -1, -2, -1]])
    assert O.labels64(match, [[7], []], None, 2).tolist() == [[7, 0, -1, -1], [0, 0, -1, -1]]
    assert O.labels64(match, [[7], []], np.array([[0, 1], [1, 0]]), 2).tolist() == [[-1, 0, -1, -1], [0, -1, -1, -1]]
    assert O.pool64(np.zeros((2, 0, 4)), gts, 1).tolist() == [[[1, 2, 3, 4]], [[0, 0, 1, 1]]]


# ================================================================================================================ GPU

def _dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def _gt_dev(gts):
    return ops.cat_boxes([_dev(g).reshape(-1, 4) for g in gts])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EXACT_CASES))
def test_match_kernels_equal_the_reference_bit_for_bit(name):
    """Exact regime: box_best_per_gt_kernel + box_match_kernel equal match64(guard = 0) on every candidate for the three
    threshold pairs with and without the low-quality restore, and box_encode_matched_kernel's `matched` output is the
    gather of those matches."""
    case = _exact_case(name)
    gt_cat, offs = _gt_dev(case["gts"])
    cand = _dev(case["cand"])
    coder = ops.BoxCoder(WEIGHTS[1])
    for (high, low) in THRESHOLDS:
        for allow in (False, True):
            want = _exact_want(case, high, low, allow)
            got = ops.match_boxes_hip(ops.Matcher(high, low, allow), gt_cat, offs, cand, shared=case["shared"])
            assert got.dtype == torch.int64 and tuple(got.shape) == want.shape
            got = got.cpu().numpy()
            bad = np.argwhere(got != want)
            assert bad.size == 0, (name, high, low, allow, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
            for want_targets in (True, False):
                _, mb = ops.encode_matched_hip(coder, gt_cat, offs, _dev(want, torch.int64), cand, case["shared"], want_targets=want_targets, want_matched=True)
                for n, g in enumerate(case["gts"]):
                    ref = g[np.maximum(want[n], 0)] if len(g) else np.zeros((case["M"], 4))
                    assert np.array_equal(mb[n].cpu().numpy(), ref.astype(np.float32)), (name, n)


@pytest.mark.gpu
def test_decode_kernel_equals_the_reference_bit_for_bit():
    coder = ops.BoxCoder(WEIGHTS[0], clip=CLIP)
    for i, (R, A) in enumerate(DECODE_EXACT):
        deltas, anchors = _decode_exact_case(R, A, 40 + i)
        want, _ = O.box_decode64(deltas, anchors, WEIGHTS[0])
        assert np.array_equal(want[np.isfinite(want)], want[np.isfinite(want)].astype(np.float32)) and np.isnan(want).any()
        got = ops.decode_boxes_hip(coder, _dev(deltas), _dev(anchors)).cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)), (R, A)
        assert np.array_equal(np.nan_to_num(got, nan=0.0), np.nan_to_num(want, nan=0.0).astype(np.float32)), (R, A)


@pytest.mark.gpu
def test_pool_and_labels_kernels_equal_the_reference():
    for i, (counts, P, Gpad, with_ok) in enumerate(_pool_cases()):
        gts, props, labels, match, ok = _pool_inputs(counts, P, Gpad, with_ok, 60 + i)
        gt_cat, offs = _gt_dev(gts)
        got = ops.pool_boxes_hip(_dev(props), gt_cat, offs, Gpad)
        assert np.array_equal(got.cpu().numpy(), O.pool64(props, gts, Gpad)), (counts, P, Gpad)
        lab_cat = _dev(np.concatenate(labels), torch.int64) if sum(counts) else None
        got = ops.pool_labels_hip(_dev(match, torch.int64), lab_cat, offs, None if ok is None else _dev(ok, torch.bool), P)
        assert got.dtype == torch.int64
        assert np.array_equal(got.cpu().numpy(), O.labels64(match, labels, ok, P)), (counts, P, Gpad)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GENERAL_CASES))
def test_match_encode_decode_kernels_are_within_the_reference_bounds(name):
    """General regime: every match in the acceptable set; `matched` exact; targets and decoded boxes within 2 x the
    CPU-measured constant of the float64 reference, NaN and infinities in the same places."""
    case = _general_case(name)
    gt_cat, offs = _gt_dev(case["gts"])
    cand = _dev(case["cand"])
    for (high, low) in THRESHOLDS:
        for allow in (False, True):
            got = ops.match_boxes_hip(ops.Matcher(high, low, allow), gt_cat, offs, cand, shared=case["shared"]).cpu().numpy()
            for n, gt in enumerate(case["gts"]):
                _, acc, _ = O.match64(gt, _image_cands(case, n), high, low, allow, guard=GUARD)
                _check_accept(got[n], acc, "%s image %d %s %s" % (name, n, (high, low), allow))
    worst = {}
    for weights in WEIGHTS:
        coder = ops.BoxCoder(weights, clip=CLIP)
        tg, mb = ops.encode_matched_hip(coder, gt_cat, offs, _dev(case["match"], torch.int64), cand, case["shared"], want_targets=True, want_matched=True)
        for n in range(len(case["gts"])):
            r = _matched_ref(case, n)
            assert np.array_equal(mb[n].cpu().numpy(), r)
            t, sc = O.box_encode64(r, _image_cands(case, n), weights)
            worst["encode"] = max(worst.get("encode", 0), C_ENC * _check_close(tg[n].cpu().numpy(), t, sc, C_ENC, "%s encode image %d" % (name, n)))
        if case["shared"]:
            d = case["deltas"] * np.array(weights, dtype=np.float32)
            b, sc = O.box_decode64(d, case["cand"], weights)
            got = ops.decode_boxes_hip(coder, _dev(d), cand).cpu().numpy()
            worst["decode"] = max(worst.get("decode", 0), C_DEC * _check_close(got, b, sc, C_DEC, "%s decode" % name))
    print(name, "largest |d| / (2^-24 scale):", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DET_CASES))
def test_det_candidates_kernel_is_within_the_reference_bounds(name):
    case = _det_case(name)
    coder = ops.BoxCoder(case["weights"], clip=CLIP)
    s, b, stats = ops.det_candidates_hip(coder, _dev(case["logits"]), _dev(case["deltas"]), _dev(case["rois"]), case["shape"], SCORE_THRESH, MIN_SIZE)
    stats = stats.cpu().numpy().view(np.uint32)
    rs_, rb_ = _check_det(case["ref"], s.cpu().numpy(), b.cpu().numpy(), (int(stats[0]), int(stats[1])), name)
    print(name, "kept %d, largest score |d| / (2^-24 scale) %.3f, box %.3f" % (int(stats[0]), C_SM * rs_, C_DEC * rb_))
