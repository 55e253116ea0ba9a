"""csrc/dib_roi.hip -- the five RoIAlign kernels and the two NMS passes -- against references that are more precise than
the kernels (oracle/dib_oracle.py A17): `roi_align64` / `roi_align_backward64`, the published definition in float64, and
`nms_greedy`, greedy NMS whose IoU decisions are made on exact integers.

  * exact regime: integer features and gradients, power-of-two scale, RoI corners on a 1/8-cell grid, pooled and grid
    sizes that are powers of two -- every float32 operation of any correct implementation is exact, so the kernels must
    equal the float64 reference bit for bit, forward and backward.  This is where the discontinuities of the definition
    (samples at -1, 0, H - 1, H, outside, clamped, reversed RoIs) are tested: float32 and float64 agree on the side;
  * general regime: random features and RoIs; |kernel - ref64| <= c * 2^-24 * max(H, W) * scale_elem per element, c from
    a CPU measurement of the plain fp32 torch path against the reference (C_FWD, C_BWD below);
  * NMS: integer boxes whose suppression structure loads the second pass (chains through every block boundary, whole
    blocks removed, long-range pairs into every word of a row), IoU exactly at the threshold, 0 / 0 boxes, `valid`;
  * the FPN level map at the areas where it switches level.

The CPU half pins the references (the loop definition of tests/test_detector_ops.py, roi_align_torch, hand-computed NMS
results) and asserts, on the references alone, what the GPU half relies on: the exactness condition, the edge-coverage
counts and the cap on bins that float32 may decide differently."""
import itertools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import dib_oracle as O
from detectinblur_amd.models import detector_ops as ops
from tests.test_detector_ops import _brute_roi_align, _rois

U = 2.0 ** -24                  # fp32 unit roundoff
GUARD = 64 * U                  # times max(H, W): the distance to a discontinuity below which fp32 may decide differently
NEAR_CAP = 0.01                 # at most this fraction of a case's bins may be `near`

# c of the general-regime bound c * 2^-24 * max(H, W) * scale_elem.  A MEASUREMENT of the plain fp32 torch path (never of a
# HIP kernel): test_torch_path_is_within_the_fp32_bound_and_measures_c prints, over every sampling_ratio > 0 case of
# _general_cases() (4 channels of each), the largest |roi_align_torch - roi_align64| / (2^-24 * max(H, W) * scale_elem).
# Found: forward 1.333 (the 7 x 9 map with aligned = 1; 0.58 - 1.12 on the others, 200 x 336 included, and 0.04 with the
# features offset by 100, whose weight errors cancel), backward 1.723 (50 x 68 with the offset; 0.15 - 1.57 on the others):
# the ratio does not grow with the map.  The constants below are those figures rounded up in the third digit.  The
# kernels get 4x that: they form each coordinate with three more roundings (y1 + ph * bh + (iy + 0.5) * bh / gh) than the
# torch path's y1 + (p + s) * bh, and the backward adds the order of its atomics.  Adaptive sampling has no torch path
# and uses the same c.
C_FWD_MEASURED, C_BWD_MEASURED, C_MARGIN = 1.34, 1.73, 4.0
C_FWD, C_BWD = C_FWD_MEASURED * C_MARGIN, C_BWD_MEASURED * C_MARGIN

CHANNELS = (1, 3, 4, 6, 64, 257, 260, 320)


# ------------------------------------------------------------------------------------------------------- exact regime

EX_H, EX_W, EX_N, EX_SCALE = 24, 40, 2, 0.25
EX_LEVELS = [((24, 40), 0.25), ((12, 20), 0.125), ((16, 16), 1.0 / 16), ((6, 10), 1.0 / 32)]      # level 2 gets no RoI


def _exact_configs():
    """(pooled, sampling_ratio, aligned); sampling_ratio 0 = adaptive, with RoI sizes that give grids of 1, 2 or 4."""
    return list(itertools.product((1, 2, 4), (1, 2, 4, 0), (0, 1)))


def _exact_rois(P, sr, aligned, H, W, scale, N, seed, wide=True):
    """RoIs aimed at the places the definition branches, built in feature cells after the `aligned` shift (`lo`, the bin
    size s in {1, 2, 4} cells per axis) and mapped back to image coordinates.  The first sample of an axis lies at
    lo + s / (2 g), the samples s / g apart."""
    rs = np.random.RandomState(seed)
    off = 0.5 if aligned else 0.0
    rows = []

    def g_of(s):
        return sr if sr > 0 else s

    def add(ty, tx, sy, sx, h=None, w=None):
        """first sample of the y axis at ty, of the x axis at tx"""
        ylo, xlo = ty - sy / (2.0 * g_of(sy)), tx - sx / (2.0 * g_of(sx))
        h = P * sy if h is None else h
        w = P * sx if w is None else w
        rows.append([len(rows) % N, (xlo + off) / scale, (ylo + off) / scale, (xlo + w + off) / scale, (ylo + h + off) / scale])

    def last(L, s):
        """first sample such that the last one lies at L"""
        return L - (P * g_of(s) - 1) * s / float(g_of(s))

    sizes = [(1, 1), (2, 4), (4, 2), (4, 4), (1, 4), (2, 2), (4, 1), (2, 1)]
    for n, (sy, sx) in enumerate(sizes):
        add(-1, 0, sy, sx)                                           # samples at y = -1, x = 0
        add(0, -1, sy, sx)
        add(last(H, sy), last(W, sx), sy, sx)                        # last samples at y = H, x = W
        add(H - 1, W - 1, sy, sx)                                    # first at H - 1 / W - 1, the rest at or beyond H / W
        add(last(H - 1, sy), last(W - 1, sx), sy, sx)                # last at H - 1 / W - 1 (inside, at the clamp)
        add(-1 - sy / float(g_of(sy)), -1 - sx / float(g_of(sx)), sy, sx)         # first below -1, second at -1
        add(H - 2, 3.125, sy, sx)                                    # rows run beyond H while columns stay inside
        add(rs.randint(0, 8 * (H - 4)) / 8.0, rs.randint(0, 8 * (W - 4)) / 8.0, sy, sx)     # interior, 1/8-cell grid
        add(rs.randint(0, 8 * H) / 8.0, rs.randint(-16, 8 * W) / 8.0, sy, sx)
    add(H + 2, 5, 1, 2)                                              # wholly outside: below the map, left of it, both
    add(3, -3 - 4 * P, 2, 4)
    add(H + 1.5, W + 1.25, 4, 4)
    if not aligned:
        add(5.125, 7.25, 1, 1, h=0.25, w=0.25)                       # smaller than one cell: clamped to 1 x 1
        add(2.5, W - 1.5, 1, 1, h=0.5, w=0.125)
    else:
        add(4.5, 9.25, 2, 1, w=0.0)                                  # zero width; adaptive: grid 0, no sample
        add(6.25, 20.5, 1, 2, h=0.0)
        add(8.5, 25.5, 1, 2, w=-2.0 * P)                             # reversed: x2 < x1, the samples of a row run right to left
        add(12.5, 30.25, 2, 1, w=-1.0 * P, h=-2.0 * P)
    if wide and sr > 0:
        # several times wider than the map: sample spacing 4 W / (P sr) cells; not with adaptive sampling, whose grid
        # (and count) would be 4 W / P: no power of two
        rows.append([0, (-1.5 * W + off) / scale, (3.0 + off) / scale, (2.5 * W + off) / scale, (3.0 + P + off) / scale])
        rows.append([1, (-0.5 * W + 0.5 + off) / scale, (H - 3.0 + off) / scale, (3.5 * W + 0.5 + off) / scale, (H - 3.0 + 2 * P + off) / scale])
    return np.array(rows, dtype=np.float32)


def _int_feat(shape, seed):
    return np.random.RandomState(seed).randint(-8, 9, shape).astype(np.float32)


def _exact_case(P, sr, aligned, C, levels=False):
    """feats, rois, level, scales, gout for one exact-regime configuration."""
    seed = 1000 * P + 10 * (sr + 1) + aligned
    if not levels:
        rois = _exact_rois(P, sr, aligned, EX_H, EX_W, EX_SCALE, EX_N, seed)
        feats, level, scales = [_int_feat((EX_N, C, EX_H, EX_W), seed + C)], None, [EX_SCALE]
    else:
        parts, lv = [], []
        for i, ((h, w), s) in enumerate(EX_LEVELS):
            if i == 2:
                continue
            r = _exact_rois(P, sr, aligned, h, w, s, EX_N, seed + i, wide=(i == 0))[::2 if i else 1]
            parts.append(r)
            lv += [i] * len(r)
        rois, level = np.concatenate(parts), np.array(lv, dtype=np.int32)
        perm = np.random.RandomState(seed).permutation(len(rois))
        rois, level = rois[perm], level[perm]
        feats = [_int_feat((EX_N, C, h, w), seed + C + i) for i, ((h, w), _) in enumerate(EX_LEVELS)]
        scales = [s for _, s in EX_LEVELS]
    gout = np.random.RandomState(seed + 7).randint(-8, 9, (len(rois), C, P, P)).astype(np.float32)
    return feats, rois, level, scales, gout


def _exact_refs(feats, rois, level, scales, gout, P, sr, aligned):
    """Forward and backward references of an exact-regime case, with the exactness condition asserted on them: every
    term a multiple of 2^-q, the sum of |terms| per output / per feature cell below 2^(24 - q) (so every partial sum in
    any order is a float32), the count a power of two (its division is exact), the geometry dyadic and small."""
    if level is None:
        f = O.roi_align64(feats[0], rois, scales[0], P, sr, aligned, exact=True)
        b = O.roi_align_backward64(gout, feats[0].shape, rois, scales[0], P, sr, aligned, exact=True)
        grads = [b["grad"]]
    else:
        f = O.roi_align64(feats, rois, scales, P, sr, aligned, level=level, exact=True)
        b = O.roi_align_backward64(gout, [x.shape for x in feats], rois, scales, P, sr, aligned, level=level, exact=True)
        grads = b["grad"]
    ef, eb = f["exact"], b["exact"]
    cnt = np.maximum(f["grid"][:, 0] * f["grid"][:, 1], 1)
    assert (cnt & (cnt - 1) == 0).all() and cnt.max() <= 16
    assert ef["q_geom"] <= 8 and ef["max_coord"] < 2 ** 10, ef              # coordinates: multiples of 2^-8 below 2^10
    assert ef["sum_fwd"] < 2.0 ** (24 - ef["q_fwd"]), ef
    assert eb["sum_bwd"] < 2.0 ** (24 - eb["q_bwd"]), eb
    for a in [f["out"]] + list(grads):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    return f, [g.astype(np.float32) for g in grads]


def _edge_counts(f, rois, level, aligned):
    """What the case list must contain, counted in the reference's sample coordinates."""
    n = dict.fromkeys(["y=-1", "y=0", "y=H-1", "y=H", "x=-1", "x=0", "x=W-1", "x=W", "beyond", "below", "outside", "subcell",
                       "zero", "reversed", "wide", "same_col", "adjacent_col", "far_col"], 0)
    for k in range(len(rois)):
        H, W = EX_LEVELS[0 if level is None else int(level[k])][0]
        y, x = f["y"][k], f["x"][k]
        iny, inx = (y >= -1) & (y <= H), (x >= -1) & (x <= W)
        for name, v, t in (("y=-1", y, -1), ("y=0", y, 0), ("y=H-1", y, H - 1), ("y=H", y, H), ("x=-1", x, -1), ("x=0", x, 0),
                           ("x=W-1", x, W - 1), ("x=W", x, W)):
            n[name] += int((v == t).sum())
        if iny.any() and inx.any():
            n["beyond"] += int(((y > H).any() or (x > W).any()))
            n["below"] += int(((y < -1).any() or (x < -1).any()))
        elif y.size and x.size:
            n["outside"] += 1
            assert not f["out"][k].any()
        rh, rw = f["raw"][k]
        n["subcell"] += int(not aligned and 0 < rw < 1 and 0 < rh < 1)
        n["zero"] += int(aligned and (rw == 0 or rh == 0))
        n["reversed"] += int(aligned and (rw < 0 or rh < 0))
        n["wide"] += int(rw >= 3 * W)
        if iny.any() and inx.sum() > 1:
            col = np.minimum(np.floor(np.maximum(x[inx], 0)), W - 1)
            d = np.abs(np.diff(col))
            n["same_col"] += int((d == 0).sum()); n["adjacent_col"] += int((d == 1).sum()); n["far_col"] += int((d > 1).sum())
    return n


# ----------------------------------------------------------------------------------------------------- general regime

def _fpn_boxes(rs, n, img_h, img_w):
    c = rs.uniform(0, 1, (n, 2)) * [img_w, img_h]
    wh = np.exp(rs.uniform(np.log(8), np.log(0.99 * min(img_h, img_w)), (n, 2)))
    b = np.concatenate([c - wh / 2, c + wh / 2], 1)
    return np.clip(b, 0, [img_w - 1, img_h - 1, img_w - 1, img_h - 1]).astype(np.float32)


def _fpn_level(boxes, n_levels):
    area = (boxes[:, 2] - boxes[:, 0]).astype(np.float64) * (boxes[:, 3] - boxes[:, 1])
    k = np.floor(4 + np.log2(np.sqrt(np.maximum(area, 1e-9)) / 224) + 1e-6)
    return (np.clip(k, 2, 1 + n_levels) - 2).astype(np.int32)


def _general_cases():
    """name -> dict(shapes [(N, C, H, W)], scales, P, sr, aligned, rois, level, offset).  Every C of CHANNELS, pooled 5 and
    7, sampling_ratio 0, 2 and 3, aligned 0 and 1, the RoI draw of tests/test_detector_ops.py and its FPN-like draw."""
    cases = OrderedDict()
    maps = [((2, 50, 68), 0.25), ((1, 25, 34), 0.125), ((3, 7, 9), 1.0 / 32), ((2, 13, 17), 1.0 / 16)]
    plan = [(0, 64, 7, 2, 0, 0.0), (0, 3, 7, 0, 0, 0.0), (1, 257, 5, 3, 1, 0.0), (1, 260, 7, 2, 1, 0.0), (2, 6, 5, 0, 1, 0.0),
            (3, 320, 7, 2, 0, 0.0), (3, 4, 5, 3, 0, 0.0), (0, 1, 7, 2, 0, 0.0), (0, 64, 7, 2, 0, 100.0), (1, 4, 7, 0, 0, 100.0),
            (2, 8, 7, 2, 1, 0.0), (0, 6, 5, 2, 1, 0.0)]
    for i, (m, C, P, sr, al, offset) in enumerate(plan):
        (N, H, W), s = maps[m]
        rs = np.random.RandomState(100 + i)
        cases["m%d_c%d_p%d_sr%d_a%d%s" % (m, C, P, sr, al, "_off" if offset else "")] = dict(
            shapes=[(N, C, H, W)], scales=[s], P=P, sr=sr, aligned=al, rois=_rois(rs, 60, N, H, W, s).numpy(), level=None,
            offset=offset, seed=100 + i)
    sizes = [(64, 96), (32, 48), (16, 24), (8, 12)]
    for j, (C, P, sr, al) in enumerate([(32, 7, 2, 0), (6, 5, 0, 1), (3, 7, 3, 0)]):
        rs = np.random.RandomState(200 + j)
        b = _fpn_boxes(rs, 80, 256, 384)
        rois = np.concatenate([rs.randint(0, 2, (80, 1)).astype(np.float32), b], 1)
        cases["fpn_c%d_p%d_sr%d_a%d" % (C, P, sr, al)] = dict(
            shapes=[(2, C, h, w) for h, w in sizes], scales=[0.25, 0.125, 1.0 / 16, 1.0 / 32], P=P, sr=sr, aligned=al, rois=rois,
            level=_fpn_level(b, 4), offset=0.0, seed=200 + j)
    rs = np.random.RandomState(300)                       # the real size: 800 x 1344 images at stride 4, C = 256
    b = _fpn_boxes(rs, 256, 800, 1344)
    rois = np.concatenate([np.concatenate([rs.randint(0, 2, (256, 1)).astype(np.float32), b], 1),
                           _rois(rs, 256, 2, 200, 336, 0.25).numpy()])
    cases["real_c256_p7_sr2_a0"] = dict(shapes=[(2, 256, 200, 336)], scales=[0.25], P=7, sr=2, aligned=0, rois=rois, level=None,
                                        offset=0.0, seed=300)
    return cases


def _general_inputs(case, max_c=None):
    rs = np.random.RandomState(case["seed"] + 5000)
    feats = [(rs.randn(*s) + case["offset"]).astype(np.float32) for s in case["shapes"]]
    gout = rs.randn(len(case["rois"]), case["shapes"][0][1], case["P"], case["P"]).astype(np.float32)
    if max_c is not None:       # channels are independent and share the geometry: a slice keeps the CPU half small
        feats, gout = [f[:, :max_c] for f in feats], gout[:, :max_c]
    return feats, gout


def _refs(case, feats, gout, rois=None, **kw):
    """(forward dict, backward dict) of a case (or of the RoIs `rois` of it), guard in cells of each RoI's level."""
    sel = slice(None) if rois is None else rois
    r, lv = case["rois"][sel], (None if case["level"] is None else case["level"][sel])
    L = max(max(s[2], s[3]) for s in case["shapes"])          # one guard per case: that of its largest level
    args = (r, case["scales"] if lv is not None else case["scales"][0], case["P"], case["sr"], case["aligned"])
    f = None if feats is None else O.roi_align64(feats if lv is not None else feats[0], *args, level=lv, guard=GUARD * L, **kw)
    shapes = [x.shape for x in feats] if feats is not None else case["gshapes"]
    b = None if gout is None else O.roi_align_backward64(gout[sel], shapes if lv is not None else shapes[0], *args, level=lv,
                                                         guard=GUARD * L, **kw)
    if b is not None and lv is None:
        b["grad"], b["gscale"] = [b["grad"]], [b["gscale"]]
    return f, b


def _roi_L(case):
    """max(H, W) of the level each RoI pools from."""
    lv = np.zeros(len(case["rois"]), dtype=np.int64) if case["level"] is None else case["level"]
    return np.array([max(case["shapes"][int(l)][2:]) for l in lv], dtype=np.float64)


def _variants(case, f):
    """For the RoIs with a `near` bin: the alternatives a float32 evaluation may arrive at (the samples within the guard
    inside / outside, the neighbouring grid size per axis) as (force, grid) pairs, and the RoIs' indices."""
    ks = np.flatnonzero(f["near"].any(axis=(1, 2)))
    g, a = f["grid"][ks], f["grid_alt"][ks]
    grids = [g, np.stack([a[:, 0], g[:, 1]], 1), np.stack([g[:, 0], a[:, 1]], 1), a]
    grids = [grids[0]] + [x for x in grids[1:] if not np.array_equal(x, g)]
    return ks, [(force, grid) for force in ("in", "out") for grid in grids]


def _check_forward(case, feats, f, got, c, what, stats):
    """Every element outside `near` within the bound of the reference; every `near` element within the bound of one of
    the alternatives."""
    L = _roi_L(case)[:, None, None, None]
    d = np.abs(got.astype(np.float64) - f["out"])
    bound = c * U * L * f["scale"]
    near = np.broadcast_to(f["near"][:, None], d.shape)
    bad = (d > bound) & ~near
    ratio = float((d[~near] / np.maximum(bound[~near], 1e-300)).max()) if (~near).any() else 0.0
    ratio = ratio if not bad.any() else float("inf")
    if near.any():
        ks, variants = _variants(case, f)
        okn = d[ks] <= bound[ks]
        for force, grid in variants:
            case_k = dict(case, rois=case["rois"][ks], level=None if case["level"] is None else case["level"][ks])
            v, _ = _refs(case_k, feats, None, force=force, grid=grid)
            okn |= np.abs(got[ks].astype(np.float64) - v["out"]) <= c * U * L[ks] * np.maximum(v["scale"], 0)
        bad[ks] |= ~okn & near[ks]
    s = stats.setdefault(what, dict(compared=0, near=0, ratio=0.0))
    s["compared"] += d.size; s["near"] += int(near.sum()); s["ratio"] = max(s["ratio"], ratio)
    assert not bad.any(), "%s forward: %d elements outside their bound, worst |d| / bound %.3g at %s" % (
        what, int(bad.sum()), float((d / np.maximum(bound, 1e-300))[bad].max()), np.argwhere(bad)[:4].tolist())


def _check_backward(case, feats_shapes, gout, f, b, got, c, what, stats):
    """Every feature cell within c * 2^-24 * max(H, W) * gscale of the reference, plus, at the cells that the samples of
    `near` bins touch, the mass |gout| / count of those samples (in any of the alternatives): what float32 may move."""
    slack = [np.zeros(s) for s in feats_shapes]
    if f["near"].any():
        ks, variants = _variants(case, f)
        gn = (gout * f["near"][:, None])[ks]
        case_k = dict(case, rois=case["rois"][ks], level=None if case["level"] is None else case["level"][ks], gshapes=feats_shapes)
        for force, grid in variants:
            if force == "in":
                _, v = _refs(case_k, None, gn, force=force, grid=grid)
                for sl, x in zip(slack, v["gscale"]):
                    sl += x
    for lv, (g, ref, sc, sl) in enumerate(zip(got, b["grad"], b["gscale"], slack)):
        Lv = float(max(feats_shapes[lv][2:]))
        d = np.abs(g.astype(np.float64) - ref)
        bound = c * U * Lv * sc
        bad = d > bound + sl
        clear = sl == 0
        s = stats.setdefault(what, dict(compared=0, near=0, ratio=0.0))
        s["compared"] += d.size; s["near"] += int((~clear).sum())
        if clear.any():
            s["ratio"] = max(s["ratio"], float((d[clear] / np.maximum(bound[clear], 1e-300)).max()) if not bad.any() else float("inf"))
        assert not bad.any(), "%s backward level %d: %d cells outside their bound, worst |d| / bound %.3g at %s" % (
            what, lv, int(bad.sum()), float((d / np.maximum(bound + sl, 1e-300))[bad].max()), np.argwhere(bad)[:4].tolist())


def _report(stats):
    for k, s in stats.items():
        print("%-28s compared %10d  near %7d  largest |d| / bound %.3f" % (k, s["compared"], s["near"], s["ratio"]))


# ---------------------------------------------------------------------------------------------------------- NMS cases

def _grid_boxes(n, size=3, pitch=4, per_row=128, x0=0, y0=0):
    """n disjoint size x size boxes on a grid."""
    i = np.arange(n)
    x, y = x0 + (i % per_row) * pitch, y0 + (i // per_row) * pitch
    return np.stack([x, y, x + size, y + size], 1).astype(np.int64)


def _chain(n):
    """10 x 10 boxes stepped by 3: IoU 7/13 with the neighbour, 4/16 with the next one, 1/19 with the third."""
    x = 3 * np.arange(n)
    return np.stack([x, 0 * x, x + 10, 0 * x + 10], 1).astype(np.int64)


CHAIN_N = (64, 65, 127, 128, 1024, 1025, 4096, 4097, 16384)

AT_THR = np.array([[0, 0, 3, 2], [1, 0, 4, 2]])           # intersection 4, union 8: IoU = 0.5 exactly, not > 0.5
ABOVE_THR = np.array([[0, 0, 10, 10], [3, 0, 13, 10]])    # 70 / 130


def _threshold_set():
    """13000 disjoint boxes with the two pairs above placed in one block, in adjacent blocks and 200 blocks apart."""
    n = 13000
    b = _grid_boxes(n, y0=100)
    at, above, at_i, above_j = [(5, 40), (60, 70), (130, 130 + 200 * 64)], [(6, 41), (61, 71), (131, 131 + 200 * 64)], [], []
    for m, ((i, j), (k, l)) in enumerate(zip(at, above)):
        b[[i, j]] = AT_THR + [40 * m, 0, 40 * m, 0]
        b[[k, l]] = ABOVE_THR + [40 * m, 20, 40 * m, 20]
        above_j.append(l)
    return b, sorted(set(range(n)) - set(above_j))


def _suppress_all(n, seed):
    rs = np.random.RandomState(seed)
    b = np.tile(np.array([[0, 0, 100, 100]]), (n, 1))
    b[1:, 0] = rs.randint(0, 20, n - 1)                   # IoU with box 0 >= 0.8
    b[1:, 1] = rs.randint(0, 5, n - 1)
    return b


def _long_range_sets(n, seed, max_sets=10):
    """Box sets [B, n, 4], all boxes disjoint except pairs (i, j > i) where j duplicates i (and is removed).  Over the sets
    there is a pair for every (row within its block i % 64, word j // 64 > i // 64): every thread of nms_reduce_kernel ORs a
    non-zero word of every row slot it holds.  The boxes left over form triples i, j, l of the chain geometry (j removed by
    i, so l, which only j would remove, survives).  Returns (boxes, removed positions per set, number of regions)."""
    rs = np.random.RandomState(seed)
    nblk = n // 64
    todo = [(r, w) for r in range(64) for w in range(1, nblk)]
    rs.shuffle(todo)
    sets, removed = [], []
    while todo and len(sets) < max_sets:
        b = _grid_boxes(n, y0=100)
        free = np.ones(n, dtype=bool)
        rem, rest = [], []
        for r, w in todo:
            js = np.flatnonzero(free[w * 64:(w + 1) * 64])
            cand = np.flatnonzero(free[r:w * 64:64])
            if js.size == 0 or cand.size == 0:
                rest.append((r, w))
                continue
            i, j = r + 64 * cand[rs.randint(cand.size)], w * 64 + js[rs.randint(js.size)]
            free[[i, j]] = False
            b[j] = b[i]
            rem.append(j)
        idle = np.flatnonzero(free)
        for m in range(min(len(idle) // 3, 40)):
            i, j, l = sorted(rs.choice(idle[3 * m:3 * m + 3], 3, replace=False))
            b[[i, j, l]] = _chain(3) + [40 * m, 0, 40 * m, 0]
            rem.append(j)
        sets.append(b); removed.append(sorted(rem))
        todo = rest
    assert not todo, "regions left uncovered: %d" % len(todo)
    return np.stack(sets), removed, 64 * (nblk - 1)


def _degenerate_set():
    """Ordinary boxes with zero-area and negative-size boxes between them, lying inside the ordinary ones."""
    b = [[0, 0, 20, 20], [5, 5, 5, 15], [2, 0, 20, 20], [5, 5, 15, 5], [7, 7, 7, 7], [7, 7, 7, 7], [15, 15, 5, 5], [15, 15, 5, 5],
         [0, 0, 20, 19], [12, 3, 4, 9], [3, 12, 9, 4], [40, 40, 60, 60], [50, 50, 50, 50], [41, 40, 60, 60]]
    return np.array(b, dtype=np.int64), [0, 1, 3, 4, 5, 6, 7, 9, 10, 11, 12]


def _dense(n, seed):
    """Integer boxes clustered so that 10 - 30 % of all pairs have IoU > 0.5."""
    rs = np.random.RandomState(seed)
    c = rs.randint(0, 40, (n, 2))
    s = rs.randint(40, 64, (n, 2))
    return np.concatenate([c, c + s], 1).astype(np.int64)


def _sets_on(device, boxes, valid, thr):
    """ops.nms_sets_sorted on one set or a batch -> list of kept-position lists, with the padded tail checked."""
    b = torch.tensor(np.asarray(boxes, dtype=np.float32), device=device)
    if b.dim() == 2:
        b = b[None]
    v = None if valid is None else torch.tensor(np.asarray(valid, dtype=bool).reshape(b.shape[:2]), device=device)
    keep, count = ops.nms_sets_sorted(b, v, thr)
    keep, count = keep.cpu().numpy(), count.cpu().numpy()
    assert keep.shape == tuple(b.shape[:2]) and count.shape == (b.shape[0],)
    out = []
    for i in range(b.shape[0]):
        assert not keep[i, count[i]:].any(), "keep[b, count[b]:] must be 0"
        out.append(keep[i, :count[i]].tolist())
    return out


def _nms_by_score(device, boxes, thr, seed):
    """The same set through ops.nms: shuffled, with distinct scores that restore the order -> kept positions in the
    original (score) order."""
    n = len(boxes)
    perm = np.random.RandomState(seed).permutation(n)                  # shuffled[p] = boxes[perm[p]]
    scores = np.empty(n, dtype=np.float32)
    scores[:] = (n - perm).astype(np.float32)                          # integers < 2^24: distinct in float32
    got = ops.nms(torch.tensor(boxes[perm].astype(np.float32), device=device), torch.tensor(scores, device=device), thr)
    return perm[got.cpu().numpy()].tolist()


# ------------------------------------------------------------------------------------------------------------ FPN map

def _level_boxes():
    """Boxes with sqrt(area) = 224 * 2^j exactly, j = -3..2 (a square and a 1 : 4 rectangle), and one grid step below and
    above each; the expected level index on a 4-level pyramid (k = 2..5) from integers: the largest k with
    area * 4^(4 - k) >= 224^2."""
    boxes, want, exact = [], [], []
    for j in range(-3, 3):
        side = 224 * 2 ** j if j >= 0 else 224 // 2 ** -j
        for w, h in ((side, side), (side // 2, side * 2)):
            for dw in (-1, 0, 1):
                ww = w + dw
                boxes.append([3, 5, 3 + ww, 5 + h])
                area = ww * h
                k = max(kk for kk in range(-8, 12) if area * 4 ** (12 - kk) >= 224 * 224 * 4 ** 8)
                want.append(min(max(k, 2), 5) - 2)
                exact.append((dw == 0, min(max(4 + j, 2), 5) - 2))
    return np.array(boxes, dtype=np.float32), want, exact


# ================================================================================================================ CPU

def test_roi_align64_equals_the_loop_definition():
    """tests/test_detector_ops.py's case and its Python-loop float64 definition: equal to rounding of the float64 sums;
    the backward reference is the transpose (float64 autograd of the torch restatement, and <gout, out> = <grad, feat>)."""
    rs = np.random.RandomState(0)
    feat = torch.tensor(rs.randn(2, 3, 11, 13), dtype=torch.float32)
    rois = _rois(rs, 9, 2, 11, 13, 0.25)
    want = _brute_roi_align(feat, rois, 0.25, 7, 2).numpy()
    f = O.roi_align64(feat.numpy(), rois.numpy(), 0.25, 7, 2, 0)
    assert np.abs(f["out"] - want).max() <= 1e-12
    assert (f["scale"] <= np.abs(feat.numpy()).max()).all() and (f["scale"] >= np.abs(f["out"]) - 1e-12).all()
    gout = rs.randn(*want.shape).astype(np.float32)
    for sr, aligned in ((2, 0), (3, 1)):
        f64 = feat.double().requires_grad_(True)
        out = ops.roi_align_torch(f64, rois.double(), 0.25, 7, sr, bool(aligned))
        out.backward(torch.tensor(gout).double())
        b = O.roi_align_backward64(gout, feat.shape, rois.numpy(), 0.25, 7, sr, aligned)
        assert np.abs(b["grad"] - f64.grad.numpy()).max() <= 1e-12
        assert (np.abs(b["grad"]) <= b["gscale"] + 1e-12).all()
    for sr, aligned, P in ((0, 0, 7), (0, 1, 5), (3, 1, 4)):                       # adaptive grids: by the dot product
        f = O.roi_align64(feat.numpy(), rois.numpy(), 0.25, P, sr, aligned)
        g = rs.randn(*f["out"].shape).astype(np.float32)
        b = O.roi_align_backward64(g, feat.shape, rois.numpy(), 0.25, P, sr, aligned)
        assert abs((f["out"] * g).sum() - (b["grad"] * feat.numpy().astype(np.float64)).sum()) <= 1e-10
        if sr == 0:
            size = np.maximum(f["raw"], 0 if aligned else 1)
            assert np.array_equal(f["grid"], np.ceil(size / P).astype(np.int64)) and f["grid"].max() >= 2


def test_roi_align64_adaptive_grid_equals_the_fixed_grid_it_selects():
    """One RoI whose adaptive grid is 3 x 2 equals the mean of the samples the definition names, written out."""
    feat = np.random.RandomState(4).randn(1, 2, 9, 11).astype(np.float32)
    roi = np.array([[0, 1.0, 2.0, 9.0, 13.0]], dtype=np.float32)        # scale 0.5: 4 x 5.5 cells, P = 2: bins 2 x 2.75
    f = O.roi_align64(feat, roi, 0.5, 2, 0, 0)
    assert f["grid"].tolist() == [[3, 2]]
    F = feat.astype(np.float64)

    def bil(c, y, x):
        y0, x0 = int(y), int(x)
        ly, lx = y - y0, x - x0
        return ((1 - ly) * (1 - lx) * F[0, c, y0, x0] + (1 - ly) * lx * F[0, c, y0, x0 + 1] + ly * (1 - lx) * F[0, c, y0 + 1, x0]
                + ly * lx * F[0, c, y0 + 1, x0 + 1])
    for c, ph, pw in itertools.product(range(2), range(2), range(2)):
        want = sum(bil(c, 1.0 + ph * 2.75 + (iy + 0.5) * 2.75 / 3, 0.5 + pw * 2.0 + (ix + 0.5) * 2.0 / 2)
                   for iy in range(3) for ix in range(2)) / 6
        assert abs(f["out"][0, c, ph, pw] - want) <= 1e-13


@pytest.mark.parametrize("levels", [False, True])
def test_exact_regime_condition_and_edge_coverage(levels):
    """On the references alone: the exactness condition of every configuration (asserted in _exact_refs) and the counts of
    the edge situations the case list must contain, each > 0 over the configurations that admit it."""
    total = {}
    for P, sr, aligned in _exact_configs():
        feats, rois, level, scales, gout = _exact_case(P, sr, aligned, 3, levels)
        f, grads = _exact_refs(feats, rois, level, scales, gout, P, sr, aligned)
        n = _edge_counts(f, rois, level, aligned)
        for k, v in n.items():
            total[(k, aligned, sr > 0)] = total.get((k, aligned, sr > 0), 0) + v
        must = ["y=-1", "y=0", "y=H-1", "y=H", "x=-1", "x=0", "x=W-1", "x=W", "outside"]
        must += ["beyond", "below"] if P * sr != 1 else []           # one sample per RoI cannot be both inside and outside
        must += ["zero", "reversed"] if aligned else ["subcell"]
        must += ["wide"] if sr > 0 else []
        assert all(n[k] > 0 for k in must), (P, sr, aligned, sorted(n.items()))
        if level is not None:
            assert set(level.tolist()) == {0, 1, 3}
        assert (rois[:, 0] == 1).any() and (rois[:, 0] == 0).any()
    # neighbouring samples of one row in the same column, in adjacent columns and (fixed grids only: the adaptive grid
    # of this regime puts the samples exactly one cell apart) more than one column apart
    for aligned, fixed in itertools.product((0, 1), (False, True)):
        keys = ("same_col", "adjacent_col", "far_col") if fixed else ("same_col", "adjacent_col")
        assert all(total[(k, aligned, fixed)] > 0 for k in keys), (aligned, fixed, total)


def test_exact_regime_torch_path_equals_the_reference():
    """In the exact regime the fp32 torch restatement equals the float64 reference bit for bit as well (fixed grids)."""
    for P, sr, aligned in _exact_configs():
        if sr == 0:
            continue
        feats, rois, level, scales, gout = _exact_case(P, sr, aligned, 6)
        f, grads = _exact_refs(feats, rois, level, scales, gout, P, sr, aligned)
        x = torch.tensor(feats[0]).requires_grad_(True)
        out = ops.roi_align_torch(x, torch.tensor(rois), scales[0], P, sr, bool(aligned))
        out.backward(torch.tensor(gout))
        assert np.array_equal(out.detach().numpy(), f["out"].astype(np.float32)), (P, sr, aligned)
        assert np.array_equal(x.grad.numpy(), grads[0]), (P, sr, aligned)


def _torch_path(case, feats, gout):
    """roi_align_torch forward and autograd backward of a case, per level and in chunks of RoIs (it gathers feat[b])."""
    K = len(case["rois"])
    out = np.zeros(gout.shape, dtype=np.float32)
    grads = []
    lvl = np.zeros(K, dtype=np.int64) if case["level"] is None else case["level"]
    for lv, f in enumerate(feats):
        x = torch.tensor(f).requires_grad_(True)
        idx = np.flatnonzero(lvl == lv)
        for s0 in range(0, idx.size, 64):
            part = idx[s0:s0 + 64]
            o = ops.roi_align_torch(x, torch.tensor(case["rois"][part]), case["scales"][lv], case["P"], case["sr"], bool(case["aligned"]))
            o.backward(torch.tensor(gout[part]))
            out[part] = o.detach().numpy()
        grads.append(np.zeros(f.shape, dtype=np.float32) if x.grad is None else x.grad.numpy())
    return out, grads


def test_near_cap_holds_for_every_general_case():
    """The guard is a condition: at most 1 % of the bins of any case lie within 64 * 2^-24 * max(H, W) of a discontinuity
    (or, with adaptive sampling, have size / pooled that close to an integer).  On the reference alone."""
    for name, case in _general_cases().items():
        feats, gout = _general_inputs(case, max_c=1)
        f, _ = _refs(case, feats, None)
        assert f["near"].mean() <= NEAR_CAP, (name, f["near"].mean())
        if case["sr"] == 0:
            assert f["grid"].max() >= 2 and len(set(map(tuple, f["grid"].tolist()))) > 1, name


def test_torch_path_is_within_the_fp32_bound_and_measures_c():
    """roi_align_torch (plain fp32) against roi_align64 on every sampling_ratio > 0 case: within the bound the kernels are
    held to, and the largest ratio is the measurement C_FWD_MEASURED / C_BWD_MEASURED quote (it must not exceed them:
    c = 4 x the measured constant, not 4 x an older one)."""
    stats, worst = {}, {"fwd": 0.0, "bwd": 0.0}
    for name, case in _general_cases().items():
        if case["sr"] <= 0:
            continue
        feats, gout = _general_inputs(case, max_c=4)
        f, b = _refs(case, feats, gout)
        out, grads = _torch_path(case, feats, gout)
        shapes = [x.shape for x in feats]
        st = {}
        _check_forward(case, feats, f, out, C_FWD, "torch fwd", st)
        _check_backward(case, shapes, gout, f, b, grads, C_BWD, "torch bwd", st)
        print("%-24s fwd ratio / c %.3f  bwd ratio / c %.3f  near bins %d" % (name, st["torch fwd"]["ratio"], st["torch bwd"]["ratio"],
                                                                           int(f["near"].sum())))
        worst["fwd"] = max(worst["fwd"], st["torch fwd"]["ratio"] * C_FWD)
        worst["bwd"] = max(worst["bwd"], st["torch bwd"]["ratio"] * C_BWD)
    print("measured constants: forward %.3f, backward %.3f" % (worst["fwd"], worst["bwd"]))
    assert worst["fwd"] <= C_FWD_MEASURED and worst["bwd"] <= C_BWD_MEASURED, worst


def test_near_bins_cannot_hide_garbage():
    """A RoI with a sample row 1e-7 beyond y = H: float64 calls it outside, float32 may call it inside.  The check accepts
    either evaluation and nothing else."""
    H, W = 12, 16
    feat = (np.random.RandomState(8).randn(1, 2, H, W) + 3).astype(np.float32)
    y2 = np.float32(4 * (H + 0.25 + 2e-6))                             # P = 1, sr = 2: samples at y2 - 0.75 h, y2 - 0.25 h
    rois = np.array([[0, 8.0, 4 * (H - 0.75), 24.0, y2]], dtype=np.float32)
    case = dict(shapes=[feat.shape], scales=[0.25], P=1, sr=2, aligned=0, rois=rois, level=None)
    f, _ = _refs(case, [feat], None)
    assert f["near"].all() and (f["y"][0] > H).sum() == 1
    inside, _ = _refs(case, [feat], None, force="in")
    assert np.abs(inside["out"] - f["out"]).min() > 0.1
    for got in (f["out"], inside["out"]):
        _check_forward(case, [feat], f, got.astype(np.float32), C_FWD, "x", {})
    for wrong in (0.5 * (f["out"] + inside["out"]), f["out"] * 1.01, inside["out"] + 0.01):
        with pytest.raises(AssertionError):
            _check_forward(case, [feat], f, wrong.astype(np.float32), C_FWD, "x", {})


def test_nms_greedy_hand_computed_cases():
    assert O.nms_greedy(_chain(9), None, 0.5) == [0, 2, 4, 6, 8]            # 7/13 removes the neighbour, 4/16 does not
    assert O.nms_greedy(_chain(9), None, 0.2) == [0, 3, 6]                  # 4/16 = 0.25 > 0.2 as well; 10/190 is not
    assert O.nms_greedy(_chain(9), None, 0.25) == [0, 2, 4, 6, 8]           # 0.25 > 0.25 is false
    assert O.nms_greedy(AT_THR, None, 0.5) == [0, 1] and O.nms_greedy(ABOVE_THR, None, 0.5) == [0]
    assert O.nms_greedy(AT_THR, None, float(np.nextafter(np.float32(0.5), np.float32(0)))) == [0]
    assert O.nms_greedy(_chain(5), [True, False, True, True, True], 0.2) == [0, 3]      # 0 removes 2 (4/16), 3 removes 4 (7/13)
    assert O.nms_greedy(_chain(5), [True, True, False, True, True], 0.5) == [0, 3]      # 1 removed by 0, 2 invalid: 3 survives
    assert O.nms_greedy(_chain(4), [False, True, True, True], 0.5) == [1, 3]            # an invalid box removes nothing
    assert O.nms_greedy(_chain(4), [False] * 4, 0.5) == [] and O.nms_greedy(np.zeros((0, 4)), None, 0.5) == []
    b, keep = _degenerate_set()
    assert O.nms_greedy(b, None, 0.5) == keep
    # 7/13 against float32 thresholds on both sides of it: one correctly rounded division decides
    q = np.float32(7) / np.float32(13)
    assert O.nms_greedy(ABOVE_THR, None, float(q)) == [0, 1]
    assert O.nms_greedy(ABOVE_THR, None, float(np.nextafter(q, np.float32(0)))) == [0]


def test_cpu_nms_path_equals_nms_greedy():
    """box_iou / _nms_torch on the CPU (the fp32 expression of torchvision) agree with the integer rule on every kind of
    case, the 0 / 0 and negative-size boxes included: that is what the kernel is then required to reproduce."""
    b, keep = _degenerate_set()
    iou = ops.box_iou(torch.tensor(b, dtype=torch.float32), torch.tensor(b, dtype=torch.float32)).numpy()
    assert np.isnan(iou[4, 5]) and np.isnan(iou[4, 4]) and not (iou[[1, 3, 4, 5, 6, 7, 9, 10, 12]] > 0).any()
    cases = [(b, None, 0.5), (_chain(200), None, 0.5), (_chain(130), None, 0.2), (AT_THR, None, 0.5), (ABOVE_THR, None, 0.5),
             (_dense(300, 1), None, 0.5), (_dense(300, 2), None, 0.7), (_suppress_all(300, 3), None, 0.5), (_grid_boxes(300), None, 0.5),
             (_dense(300, 4), np.random.RandomState(4).rand(300) > 0.3, 0.5)]
    sets, removed, _ = _long_range_sets(256, 5)
    cases += [(s, None, 0.5) for s in sets]
    for boxes, valid, thr in cases:
        want = O.nms_greedy(boxes, valid, thr)
        assert _sets_on("cpu", boxes, valid, thr) == [want]
        if valid is None:
            assert _nms_by_score("cpu", boxes, thr, 1) == want
    for s, r in zip(sets, removed):
        assert O.nms_greedy(s, None, 0.5) == sorted(set(range(256)) - set(r))
    fill = np.triu(ops.box_iou(*(torch.tensor(_dense(1000, 16), dtype=torch.float32),) * 2).numpy() > 0.5, 1).sum() / (1000 * 999 / 2)
    assert 0.1 <= fill <= 0.3, fill


def test_structured_nms_cases_have_the_stated_structure():
    b, keep = _threshold_set()
    assert O.nms_greedy(b, None, 0.5) == keep and len(keep) == 13000 - 3
    for n in (1024, 4096):
        sets, removed, regions = _long_range_sets(n, n)
        hit = set()
        for s, r in zip(sets, removed):
            for j in r:
                i = int(np.flatnonzero((s[:j] == s[j]).all(axis=1))[0]) if (s[:j] == s[j]).all(axis=1).any() else None
                if i is not None:
                    hit.add((i % 64, j // 64))
        assert len({(r, w) for r, w in hit if w > 0}) >= regions, (n, len(hit), regions)
    assert O.nms_greedy(_suppress_all(5000, 1), None, 0.5) == [0]
    assert O.nms_greedy(_grid_boxes(2000), None, 0.5) == list(range(2000))


def test_level_boxes_reference_is_the_fpn_rule():
    boxes, want, exact = _level_boxes()
    assert sorted(set(want)) == [0, 1, 2, 3]
    for w, (is_exact, lvl) in zip(want, exact):
        assert not is_exact or w == lvl
    area = (boxes[:, 2] - boxes[:, 0]).astype(np.float64) * (boxes[:, 3] - boxes[:, 1])
    k = np.clip(np.floor(4 + np.log2(np.sqrt(area) / 224)), 2, 5) - 2        # float64: 0.0008 away from a switch at least
    assert k.tolist() == want


def test_nms_docstring_states_the_truncation():
    assert "16384" in ops.nms.__doc__


# ================================================================================================================ GPU

def _cl(x):
    return x.contiguous(memory_format=torch.channels_last)


def _misaligned_cl(x):
    """A channels-last copy of x whose data_ptr() is 4 bytes off a 16-byte boundary (a view into a flat buffer)."""
    N, C, H, W = x.shape
    flat = torch.empty(x.numel() + 8, dtype=torch.float32, device=x.device)
    start = 1 + (-(flat.data_ptr() // 4) % 4)
    v = flat[start:start + x.numel()].view(N, H, W, C).permute(0, 3, 1, 2)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4 and ops._is_nhwc(v)
    return v


def _run_kernels(feats, rois, level, scales, gout, P, sr, aligned):
    """Every kernel path that accepts the configuration -> {name: (out, [grad per level])} as numpy arrays.
      planar         roi_align_fwd_kernel / roi_align_bwd_kernel (per level for a pyramid)
      nhwc           roi_align_fwd_nhwc_sr_kernel<2> when sr == 2 and C % 4 == 0, else roi_align_fwd_nhwc_kernel;
                     roi_align_bwd_nhwc_kernel
      nhwc_generic   roi_align_fwd_nhwc_kernel forced on a vectorisable shape through a misaligned base pointer"""
    dev = "cuda"
    C = feats[0].shape[1]
    r, g = torch.tensor(rois, device=dev), torch.tensor(gout, device=dev)
    lv = None if level is None else torch.tensor(level, dtype=torch.int32, device=dev)
    res = {}
    xs = [torch.tensor(f, device=dev).requires_grad_(True) for f in feats]
    out = torch.zeros(gout.shape, device=dev)
    for i, x in enumerate(xs):
        idx = torch.arange(len(rois), device=dev) if lv is None else torch.where(lv == i)[0]
        o = ops._RoIAlignHIP.apply(x, r[idx], scales[i], P, sr, aligned)
        o.backward(g[idx])
        out[idx] = o.detach()
    res["planar"] = (out.cpu().numpy(), [(torch.zeros_like(x) if x.grad is None else x.grad).cpu().numpy() for x in xs])
    if C > 1 and P <= 7:
        variants = [("nhwc", _cl)] + ([("nhwc_generic", _misaligned_cl)] if sr == 2 and C % 4 == 0 else [])
        for name, fmt in variants:
            xs = [fmt(torch.tensor(f, device=dev)).requires_grad_(True) for f in feats]
            if lv is None:
                o = ops.roi_align(xs[0], r, scales[0], P, sr, aligned)
            else:
                o = ops._RoIAlignNHWC.apply(r, lv, scales, P, sr, aligned, *xs)
            o.backward(g)
            assert all(x.grad.is_contiguous(memory_format=torch.channels_last) for x in xs)
            res[name] = (o.detach().cpu().numpy(), [x.grad.cpu().numpy() for x in xs])
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [False, True])
@pytest.mark.parametrize("C", CHANNELS)
def test_roi_align_kernels_equal_the_reference_bit_for_bit(C, levels):
    """Exact regime: every kernel, forward and backward, equals roi_align64 / roi_align_backward64 with no tolerance, for
    pooled 1 / 2 / 4, sampling ratio 1 / 2 / 4 / adaptive, aligned 0 / 1, one level and a 4-level pyramid."""
    n = 0
    for P, sr, aligned in _exact_configs():
        feats, rois, level, scales, gout = _exact_case(P, sr, aligned, C, levels)
        f, grads = _exact_refs(feats, rois, level, scales, gout, P, sr, aligned)
        want = f["out"].astype(np.float32)
        got = _run_kernels(feats, rois, level, scales, gout, P, sr, aligned)
        assert ("nhwc" in got) == (C > 1) and ("nhwc_generic" in got) == (sr == 2 and C % 4 == 0)
        for name, (out, gr) in got.items():
            bad = np.argwhere(out != want)
            assert bad.size == 0, (name, "forward", P, sr, aligned, len(bad), bad[:4].tolist(), rois[bad[0][0]].tolist())
            for lv, (a, b) in enumerate(zip(gr, grads)):
                bad = np.argwhere(a != b)
                assert bad.size == 0, (name, "backward", P, sr, aligned, lv, len(bad), bad[:4].tolist())
            n += out.size + sum(a.size for a in gr)
    print("exact regime C=%d levels=%s: %d elements equal" % (C, levels, n))


@pytest.mark.gpu
def test_roi_align_wrapper_edges_pooled_8_and_no_rois():
    """pooled = 8 on a channels-last map (above the channels-last kernels' limit: the wrapper's planar fall-back), exact
    regime; K = 0 through every wrapper."""
    for sr, aligned in ((2, 0), (0, 1), (4, 1)):
        feats, rois, level, scales, gout = _exact_case(8, sr, aligned, 8)
        f, grads = _exact_refs(feats, rois, level, scales, gout, 8, sr, aligned)
        x = _cl(torch.tensor(feats[0], device="cuda")).requires_grad_(True)
        out = ops.roi_align(x, torch.tensor(rois, device="cuda"), scales[0], 8, sr, aligned)
        out.backward(torch.tensor(gout, device="cuda"))
        assert np.array_equal(out.detach().cpu().numpy(), f["out"].astype(np.float32)), (sr, aligned)
        assert np.array_equal(x.grad.cpu().numpy(), grads[0]), (sr, aligned)
    none = torch.zeros((0, 5), device="cuda")
    for fmt in (lambda t: t, _cl):
        x = fmt(torch.randn(2, 8, 10, 12, device="cuda")).requires_grad_(True)
        out = ops.roi_align(x, none, 0.25, 7, 2)
        assert out.shape == (0, 8, 7, 7)
        out.sum().backward()
        assert x.grad is not None and not x.grad.any()


_GENERAL_STATS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_general_cases()))
def test_roi_align_kernels_are_within_the_fp32_bound(name):
    """General regime: every element outside `near` within c * 2^-24 * max(H, W) * scale_elem of the float64 reference,
    `near` elements within it of one of the alternatives; planar and channels-last forward bit-identical, generic and
    vectorised channels-last forward bit-identical."""
    case = _general_cases()[name]
    feats, gout = _general_inputs(case)
    f, b = _refs(case, feats, gout)
    assert f["near"].mean() <= NEAR_CAP
    shapes = [x.shape for x in feats]
    got = _run_kernels(feats, case["rois"], case["level"], case["scales"], gout, case["P"], case["sr"], case["aligned"])
    assert ("nhwc" in got) == (shapes[0][1] > 1)
    vec = case["sr"] == 2 and shapes[0][1] % 4 == 0
    kernel = {"planar": "planar", "nhwc": "nhwc vectorised" if vec else "nhwc generic", "nhwc_generic": "nhwc generic"}
    for k, (out, grads) in got.items():
        _check_forward(case, feats, f, out, C_FWD, kernel[k] + " fwd", _GENERAL_STATS)
        _check_backward(case, shapes, gout, f, b, grads, C_BWD, ("planar" if k == "planar" else "nhwc") + " bwd", _GENERAL_STATS)
        assert np.array_equal(out, got["planar"][0]), (name, k, "forward differs from the planar kernel's")
    print("after %s:" % name)
    _report(_GENERAL_STATS)


def _gpu_sets(boxes, valid, thr):
    return _sets_on("cuda", boxes, valid, thr)


@pytest.mark.gpu
@pytest.mark.parametrize("n", CHAIN_N)
def test_nms_chain_through_every_block_boundary(n):
    """Every decision depends on the previous one: every second box survives (thr 0.5), every third (thr 0.2)."""
    b = _chain(n)
    assert _gpu_sets(b, None, 0.5) == [list(range(0, n, 2))] == [O.nms_greedy(b, None, 0.5)]
    assert _gpu_sets(b, None, 0.2) == [list(range(0, n, 3))] == [O.nms_greedy(b, None, 0.2)]
    assert _nms_by_score("cuda", b, 0.5, n) == list(range(0, n, 2))


@pytest.mark.gpu
def test_nms_iou_exactly_at_the_threshold():
    assert _gpu_sets(AT_THR, None, 0.5) == [[0, 1]] and _gpu_sets(ABOVE_THR, None, 0.5) == [[0]]
    assert _gpu_sets(_chain(9), None, 0.25) == [[0, 2, 4, 6, 8]]
    q = np.float32(7) / np.float32(13)            # the correctly rounded quotient as the threshold: not above itself
    assert _gpu_sets(ABOVE_THR, None, float(q)) == [[0, 1]]
    assert _gpu_sets(ABOVE_THR, None, float(np.nextafter(q, np.float32(0)))) == [[0]]
    b, keep = _threshold_set()
    assert _gpu_sets(b, None, 0.5) == [keep] == [O.nms_greedy(b, None, 0.5)]
    assert _nms_by_score("cuda", b, 0.5, 3) == keep


@pytest.mark.gpu
def test_nms_whole_blocks_removed_and_nothing_removed():
    for n in (5000, 16384):
        b = _suppress_all(n, n)
        assert _gpu_sets(b, None, 0.5) == [[0]] == [O.nms_greedy(b, None, 0.5)]
        assert _nms_by_score("cuda", b, 0.5, n) == [0]
    b = _grid_boxes(16384)
    assert _gpu_sets(b, None, 0.5) == [list(range(16384))] == [O.nms_greedy(b, None, 0.5)]
    # the first box removes blocks 1 .. 100 whole and parts of block 0 and 101; the rest is disjoint
    b = _grid_boxes(16384, y0=200)
    b[1:6500] = _suppress_all(6499, 2)
    b[0] = [0, 0, 100, 100]
    b[3] = [300, 0, 303, 3]
    want = O.nms_greedy(b, None, 0.5)
    assert want[:3] == [0, 3, 6500] and _gpu_sets(b, None, 0.5) == [want]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1024, 4096, 16384])
def test_nms_long_range_pairs_into_every_word_of_every_row(n):
    sets, removed, regions = _long_range_sets(n, n)
    got = _gpu_sets(sets, None, 0.5)
    for s, r, g in zip(sets, removed, got):
        want = sorted(set(range(n)) - set(r))
        assert g == want
    assert got[0] == O.nms_greedy(sets[0], None, 0.5)
    print("n=%d: %d sets cover %d (row, word) regions" % (n, len(sets), regions))


@pytest.mark.gpu
def test_nms_zero_area_and_negative_size_boxes():
    b, keep = _degenerate_set()
    assert _gpu_sets(b, None, 0.5) == [keep] == _sets_on("cpu", b, None, 0.5)
    rs = np.random.RandomState(9)
    big = _dense(3000, 9)
    deg = rs.rand(3000) < 0.3
    kind = rs.randint(0, 3, 3000)
    big[deg & (kind == 0), 2] = big[deg & (kind == 0), 0]                       # zero width
    big[deg & (kind == 1), 3] = big[deg & (kind == 1), 1] - 5                   # negative height
    big[deg & (kind == 2), 2:] = big[deg & (kind == 2), :2] - [3, 7]            # both negative: a positive "area"
    want = O.nms_greedy(big, None, 0.5)
    assert set(np.flatnonzero(deg).tolist()) <= set(want)                       # never removed
    assert _gpu_sets(big, None, 0.5) == [want]


@pytest.mark.gpu
def test_nms_valid_masks():
    rs = np.random.RandomState(12)
    n = 700
    boxes = np.stack([_dense(n, 20), _chain(n), _dense(n, 21), _chain(n)])
    valid = np.stack([rs.rand(n) > 0.3, np.arange(n) % 2 == 1, np.zeros(n, dtype=bool), np.ones(n, dtype=bool)])
    got = _gpu_sets(boxes, valid, 0.5)
    want = [O.nms_greedy(boxes[i], valid[i], 0.5) for i in range(4)]
    assert got == want and want[2] == []
    assert want[1] == list(range(1, n, 2))          # the invalid even boxes would have removed every odd one (7/13)
    assert _gpu_sets(boxes, None, 0.5) == [O.nms_greedy(boxes[i], None, 0.5) for i in range(4)]


@pytest.mark.gpu
def test_nms_limits():
    b = _chain(16385)
    t = torch.tensor(b[None].astype(np.float32), device="cuda")
    with pytest.raises(ValueError):
        ops.nms_sets_sorted(t, None, 0.5)
    assert _gpu_sets(b[:16384], None, 0.5) == [list(range(0, 16384, 2))]
    # ops.nms keeps only the 16384 best boxes: the box with the lowest score takes no part
    perm = np.random.RandomState(5).permutation(16385)
    scores = (16385 - perm).astype(np.float32)
    got = ops.nms(torch.tensor(b[perm].astype(np.float32), device="cuda"), torch.tensor(scores, device="cuda"), 0.5)
    assert perm[got.cpu().numpy()].tolist() == O.nms_greedy(b[:16384], None, 0.5) == list(range(0, 16384, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1000, 4000, 9000])
def test_nms_dense_random(n):
    """One dense randomised case per nms_reduce_kernel instantiation (16, 64 and 256 words per row)."""
    for thr, seed in ((0.5, n), (0.7, n + 1)):
        b = _dense(n, seed)
        want = O.nms_greedy(b, None, thr)
        assert _gpu_sets(b, None, thr) == [want]
        assert _nms_by_score("cuda", b, thr, seed) == want


@pytest.mark.gpu
def test_fpn_level_map_at_the_areas_where_it_switches():
    """A pyramid whose level l is the constant l: the pooled output names the level.  Exact areas (sqrt = 224 * 2^j) go to
    clamp(4 + j); the per-level planar path, the channels-last one-launch path and the integer rule agree on all, and the
    two paths' outputs are bit-identical.  The output is l up to the float32 rounding of the bilinear sum (the four
    weights of a sample are rounded products of rounded 1 - l terms and do not add up to 1 exactly): per sample 2 roundings
    in the weights' factors, 4 in their products, 4 in the products with l and 3 in the sum, then 3 + 1 for the mean of the
    four samples: 17 * 2^-24 * l, asserted as 32 * 2^-24 * l; level 0 is exactly 0."""
    boxes, want, exact = _level_boxes()
    sizes = [(512, 512), (256, 256), (128, 128), (64, 64)]
    pool = ops.MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)
    bx = [torch.tensor(boxes[::2], device="cuda"), torch.tensor(boxes[1::2], device="cuda")]
    expect = np.array(want[::2] + want[1::2], dtype=np.float64)
    outs = []
    for fmt in (torch.contiguous_format, torch.channels_last):
        fs = OrderedDict((str(i), torch.full((2, 4, h, w), float(i), device="cuda").contiguous(memory_format=fmt))
                         for i, (h, w) in enumerate(sizes))
        out = pool(fs, bx, [(2048, 2048), (2048, 2048)]).cpu().numpy()
        assert out.shape == (len(want), 4, 7, 7)
        d = np.abs(out.astype(np.float64) - expect[:, None, None, None]).max(axis=(1, 2, 3))
        print(fmt, "levels", np.rint(out[:, 0, 0, 0]).astype(int).tolist(), "expected", expect.astype(int).tolist(),
              "largest |out - l| / (2^-24 l)", float((d / (U * np.maximum(expect, 1))).max()))
        assert (d <= 32 * U * expect).all(), (fmt, np.flatnonzero(d > 32 * U * expect).tolist(), out[:, 0, 0, 0].tolist(), expect.tolist())
        outs.append(out)
    assert np.array_equal(outs[0], outs[1])
    for w, (is_exact, lvl) in zip(want, exact):
        assert not is_exact or w == lvl
