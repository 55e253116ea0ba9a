"""Exact references for everything that selects by score -- csrc/dib_topk.hip and its four call sites (the RPN's per-level
selection and last ranking in models/rpn.py: _filter, the per-class sort and last ranking in models/roi_heads.py:
_detections_hip) -- with the input generators tests/test_selection_gpu.py runs on the device, and the CPU checks of both.

The references are integers and stable sorts only:

  topk_stable       per level torch.sort(descending=True, stable=True) on the CPU, padded as the kernel pads;
  detections_ref    postprocess_detections with every tie broken by (class, RoI index), NMS by oracle nms_greedy;
  rpn_filter_ref    filter_proposals with every tie broken by (level, index), NMS by oracle nms_greedy.

The generators produce scores and boxes that are known exactly (softmax rows equal to 1 / m, integer boxes whose IoUs
nms_greedy decides on integers), so the device results are compared bit for bit: no tolerance appears anywhere.  Every
generator's claim ("the k-th place lies strictly inside a tie run", "more survivors than D, all at 1.0", ...) is asserted
here on the reference alone, so a GPU test cannot pass on an input that lost its ties."""
import numpy as np
import torch
import torch.nn.functional as F

import dib_oracle as O
from detectinblur_amd.models import detector_ops as ops
from detectinblur_amd.models.roi_heads import RoIHeads
from detectinblur_amd.models.rpn import RegionProposalNetwork
from tests.test_roi_nms_reference import ABOVE_THR, AT_THR, _chain, _grid_boxes

NEG_INF = float("-inf")


# ========================================================================================================= references

def _clip(b, wh):
    """clip_boxes_to_image on [N, k, 4] with wh [N, 2] = (w, h): clamp(min=0).minimum(size); a NaN coordinate stays NaN."""
    w, h = wh[:, None, 0:1], wh[:, None, 1:2]
    x = b[..., 0::2].clamp(min=0).minimum(w)
    y = b[..., 1::2].clamp(min=0).minimum(h)
    return torch.stack((x[..., 0], y[..., 0], x[..., 1], y[..., 1]), dim=-1)


def topk_stable(values, counts, ks, K, boxes=None, clip_wh=None, min_size=0.0, offset0=0):
    """values [N, A] (CPU float32); level l = the next counts[l] columns from column `offset0` on.  Per level the first
    min(ks[l], counts[l]) places of a stable descending sort: descending score, ascending level-relative index among equal
    scores (-0 == +0), NaN first.  Returns scores [N, L, K] padded with -inf, index [N, L, K] padded with 0, and with
    `boxes` [N, A, 4]: the winners' boxes [N, L, K, 4] (clipped to clip_wh [N, 2] = (w, h) if given, padded with 0) and
    valid [N, L, K] = score > -inf and both sides >= min_size (padded with False); None, None without boxes."""
    values = torch.as_tensor(values)
    assert values.device.type == "cpu" and values.dtype == torch.float32
    N, L = values.shape[0], len(counts)
    s = torch.full((N, L, K), NEG_INF)
    ix = torch.zeros((N, L, K), dtype=torch.int64)
    ob = torch.zeros((N, L, K, 4)) if boxes is not None else None
    ov = torch.zeros((N, L, K), dtype=torch.bool) if boxes is not None else None
    off = offset0
    for l, (c, k) in enumerate(zip(counts, ks)):
        k = min(int(k), int(c), K)
        if k > 0:
            v, i = torch.sort(values[:, off:off + c], dim=1, descending=True, stable=True)
            v, i = v[:, :k], i[:, :k]
            s[:, l, :k], ix[:, l, :k] = v, i
            if boxes is not None:
                b = boxes[:, off:off + c].gather(1, i[..., None].expand(-1, -1, 4))
                if clip_wh is not None:
                    b = _clip(b, clip_wh)
                ob[:, l, :k] = b
                ov[:, l, :k] = (v > NEG_INF) & ((b[..., 2] - b[..., 0]) >= min_size) & ((b[..., 3] - b[..., 1]) >= min_size)
        off += c
    return s, ix, ob, ov


def detections_ref(scores, boxes, score_thresh, min_size, nms_thresh, D):
    """scores [R, C] (column 0 = background), boxes [R, C, 4] decoded and clipped.  Per class 1 .. C - 1: the candidates
    with score > score_thresh and both sides >= min_size (a NaN side fails), by descending score with the RoI index
    breaking ties, greedy NMS (oracle nms_greedy: integer boxes), the first d = min(D, R) survivors.  The classes'
    survivors class-major, stable sort by descending score -- equal scores stay in (class, rank) order --, the first
    min(D, total).  Returns (boxes [n, 4] float32, labels [n] int64, scores [n] float32, n)."""
    scores, boxes = np.asarray(scores, dtype=np.float32), np.asarray(boxes, dtype=np.float32)
    R, C = scores.shape
    d = min(D, R)
    cat_s, cat_b, cat_l = [np.zeros(0, np.float32)], [np.zeros((0, 4), np.float32)], [np.zeros(0, np.int64)]
    for c in range(1, C):
        s, b = scores[:, c], boxes[:, c]
        idx = np.flatnonzero((s > score_thresh) & ((b[:, 2] - b[:, 0]) >= min_size) & ((b[:, 3] - b[:, 1]) >= min_size))
        idx = idx[np.argsort(-s[idx], kind="stable")]
        idx = idx[O.nms_greedy(b[idx], None, nms_thresh)][:d]
        cat_s.append(s[idx]); cat_b.append(b[idx]); cat_l.append(np.full(idx.size, c, dtype=np.int64))
    cat_s, cat_b, cat_l = np.concatenate(cat_s), np.concatenate(cat_b), np.concatenate(cat_l)
    order = np.argsort(-cat_s, kind="stable")[:D]
    return cat_b[order], cat_l[order], cat_s[order], int(order.size)


def rpn_filter_ref(proposals, objectness, sizes, counts, pre, post, min_size, nms_thresh, with_all=False):
    """proposals [N, A, 4], objectness [N, A], sizes [N, 2] = (w, h), CPU float32.  Per (image, level): the stable
    top-min(pre, n), clipped to (w, h), flagged valid = both sides >= min_size; nms_greedy over the valid boxes in that order.
    The levels' survivors level-major, stable sort by descending score -- equal scores stay in (level, rank) order --, the
    first `post` rows.  Returns per image (boxes [count, 4], scores [count], count = min(post, survivors)); with_all: the
    scores of ALL survivors in their final order instead of the first `post` (for the structure checks)."""
    proposals, objectness, sizes = torch.as_tensor(proposals), torch.as_tensor(objectness), torch.as_tensor(sizes)
    K = max(min(pre, n) for n in counts)
    s, _, b, v = topk_stable(objectness, counts, [min(pre, n) for n in counts], K, proposals, sizes, min_size)
    s, b, v = s.numpy(), b.numpy(), v.numpy()
    out = []
    for n in range(proposals.shape[0]):
        cs, cb = [np.zeros(0, np.float32)], [np.zeros((0, 4), np.float32)]
        for l in range(len(counts)):
            keep = O.nms_greedy(b[n, l], v[n, l], nms_thresh)
            cs.append(s[n, l, keep]); cb.append(b[n, l, keep])
        cs, cb = np.concatenate(cs), np.concatenate(cb)
        order = np.argsort(-cs, kind="stable")
        if not with_all:
            order = order[:post]
        out.append((cb[order], cs[order], int(min(post, cs.size))))
    return out


# ============================================================================================ top-k: families, geometry

def topk_key(v):
    """The order-preserving 32-bit key of csrc/dib_topk.hip as integers: NaN the largest, both zeros one key, the negative
    half inverted.  Only the structure checks below use it (which radix pass decides); the expected results never do."""
    v = np.asarray(v, dtype=np.float32)
    b = v.view(np.uint32)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    key = np.where(v == 0, np.uint32(0x80000000), key)
    return np.where(np.isnan(v), np.uint32(0xffffffff), key).astype(np.uint32)


def kth_run(vec, k):
    """(first, last) sorted places, 0-based, of the run of equal scores that holds the k-th place (place k - 1) of the
    stable descending sort.  NaNs equal each other, -0 equals +0."""
    v = torch.sort(torch.as_tensor(vec), descending=True, stable=True)[0].numpy()
    same = (v == v[k - 1]) | (np.isnan(v) & np.isnan(v[k - 1]))
    first = last = k - 1
    while first > 0 and same[first - 1]:
        first -= 1
    while last + 1 < v.size and same[last + 1]:
        last += 1
    return first, last


SAT_VALUES = np.array([1.0, 0.5, 0.25, 1.0 / 16, NEG_INF], dtype=np.float32)


def _fam_near_one(cnt, k, rs, sign=1.0):
    """1 - j 2^-24, j < 1024, with repeats; j = 0 is 1.0 itself.  Below 1 every key shares its upper 22 bits."""
    j = rs.randint(0, min(1024, max(2, cnt // 3)), cnt)
    return (sign * (1.0 - j * 2.0 ** -24)).astype(np.float32)


def _fam_middle(cnt, k, rs, sign=1.0):
    """1 - j 2^-14, j < 2048: the keys differ in bits 10 .. 20, the second pass decides."""
    j = rs.randint(0, min(2048, max(2, cnt // 3)), cnt)
    return (sign * (1.0 - j * 2.0 ** -14)).astype(np.float32)


def _fam_denormal(cnt, k, rs):
    """+- m 2^-149, m < 512, both zeros among them.  Where cnt and k leave room (denormal_room): k - 1 positive denormals,
    then two to five zeros of both signs, then negative denormals, shuffled -- the k-th place is the first zero by index,
    the next place another zero."""
    hi = min(512, max(2, cnt // 3))
    if denormal_room(cnt, k):
        zeros = min(cnt - (k - 1), rs.randint(2, 6))
        neg = cnt - (k - 1) - zeros
        m = np.concatenate([rs.randint(1, hi, k - 1), np.zeros(zeros, dtype=np.int64), rs.randint(1, hi, neg)]).astype(np.uint32)
        sign = np.concatenate([np.zeros(k - 1), (np.arange(zeros) + 1) % 2, np.ones(neg)]).astype(np.uint32)
        p = rs.permutation(cnt)
        m, sign = m[p], sign[p]
    else:
        m, sign = rs.randint(0, hi, cnt).astype(np.uint32), rs.randint(0, 2, cnt).astype(np.uint32)
    return (m | (sign << np.uint32(31))).view(np.float32)


def denormal_room(cnt, k):
    return cnt >= 4 and 1 <= k <= cnt - 1


def _fam_saturated(cnt, k, rs, mode):
    """A multiset of {1, 1/2, 1/4, 1/16, -inf}, shuffled, with the k-th place of the sort strictly inside a run of 1/2
    (`inside`), on the run's last element (`last`) or on its first (`first`) wherever cnt and k leave room for that
    (saturated_room); any multiset otherwise."""
    if not saturated_room(cnt, k, mode):
        return SAT_VALUES[rs.randint(0, 5, cnt)]
    if mode == "inside":                       # places k - 2, k - 1, k all hold 1/2
        ones = rs.randint(0, k - 1)
        half = rs.randint(k + 1 - ones, cnt - ones + 1)
    elif mode == "last":                       # the run ends on place k - 1 and is at least two long
        ones = rs.randint(0, k - 1)
        half = k - ones
    else:                                      # the run starts on place k - 1 and is at least two long
        ones = k - 1
        half = rs.randint(2, cnt - ones + 1)
    rest = cnt - ones - half
    cut = np.sort(rs.randint(0, rest + 1, 2))
    v = np.concatenate([np.full(ones, 1.0), np.full(half, 0.5), np.full(cut[0], 0.25), np.full(cut[1] - cut[0], 1.0 / 16),
                        np.full(rest - cut[1], NEG_INF)]).astype(np.float32)
    return v[rs.permutation(cnt)]


def saturated_room(cnt, k, mode):
    return {"inside": 2 <= k <= cnt - 1, "last": 2 <= k <= cnt, "first": 1 <= k <= cnt - 1}[mode]


def _fam_inf_majority(cnt, k, rs):
    """A handful of finite scores (two of them tied), the rest -inf: k above the finite count takes -inf elements, by index."""
    v = np.full(cnt, NEG_INF, dtype=np.float32)
    f = min(5, cnt)
    v[rs.choice(cnt, f, replace=False)] = np.array([0.5, 1.0, 0.5, 0.25, 1.0 / 16], dtype=np.float32)[:f]
    return v


def _fam_nan(cnt, k, rs):
    """Scores on a grid of 1/4 (ties everywhere) with up to three NaNs."""
    v = (rs.randint(-4, 5, cnt) / 4.0).astype(np.float32)
    v[rs.choice(cnt, min(3, cnt // 2), replace=False)] = np.nan
    return v


def _fam_constant(cnt, k, rs):
    return np.full(cnt, 0.25, dtype=np.float32)


FAMILIES = [
    ("near_one", _fam_near_one),
    ("near_one_negated", lambda c, k, rs: _fam_near_one(c, k, rs, -1.0)),
    ("middle", _fam_middle),
    ("middle_negated", lambda c, k, rs: _fam_middle(c, k, rs, -1.0)),
    ("denormal", _fam_denormal),
    ("saturated_inside", lambda c, k, rs: _fam_saturated(c, k, rs, "inside")),
    ("saturated_last", lambda c, k, rs: _fam_saturated(c, k, rs, "last")),
    ("saturated_first", lambda c, k, rs: _fam_saturated(c, k, rs, "first")),
    ("inf_majority", _fam_inf_majority),
    ("nan", _fam_nan),
    ("constant", _fam_constant),
]
FAMILY_NAMES = [n for n, _ in FAMILIES]

LENGTHS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 8191, 8192, 8193, 16385)
KS = (0, 1, 2, 3, 1023, 1024, 1025, 2047, 2048)
MAX_K, MAX_LEVELS = 2048, 32


def geometry_pairs():
    """Every (row length, k): k in {0, 1, 2, 3, 1023, 1024, 1025, 2047, 2048, cnt - 1, cnt} where 0 <= k <= min(cnt, 2048)."""
    return [(c, k) for c in LENGTHS for k in sorted(set(KS) | {c - 1, c}) if 0 <= k <= min(c, MAX_K)]


def geometry_launches():
    """The pairs as launches of at most 32 levels, sorted by k so that a launch's K (its largest k) is not far above its
    other k: (counts, ks, [K, ...]) with K = the largest k and, where 2048 allows, K above it (every row ends in padding)."""
    pairs = sorted(geometry_pairs(), key=lambda p: (p[1], p[0]))
    out = []
    for i in range(0, len(pairs), MAX_LEVELS):
        part = pairs[i:i + MAX_LEVELS]
        top = max(max(k for _, k in part), 1)
        out.append(([c for c, _ in part], [k for _, k in part], [top] + ([top + 5] if top + 5 <= MAX_K else [])))
    return out


def family_rows(counts, ks, seed):
    """[len(FAMILIES), sum(counts)] float32: row f holds family f's vector for every (count, k) level, level after level."""
    rs = np.random.RandomState(seed)
    rows = [np.concatenate([fn(c, k, rs) for c, k in zip(counts, ks)] + [np.zeros(0, np.float32)]) for _, fn in FAMILIES]
    return np.stack(rows).astype(np.float32)


def index_boxes(N, A):
    """Integer boxes [N, A, 4] computed from the position (cheap for long rows): corners from -12 up, sides 0 .. 12, so that
    clipping to CLIP_WH = (70, 60) changes some on either side and the size test drops some (zero sides, clipped to nothing)."""
    a = np.arange(A, dtype=np.int64)[None, :] + 7 * np.arange(N, dtype=np.int64)[:, None]
    x, y = a % 97 - 12, a % 89 - 12
    return torch.tensor(np.stack([x, y, x + a % 13, y + a % 11], axis=-1).astype(np.float32))


CLIP_WH = (70.0, 60.0)

BOUNDARIES = (63, 64, 1023, 1024, 8191, 8192)
GAP = 8193          # "after a gap of more than 8192": the next equal lies beyond a whole unrolled sweep of the workgroup


def boundary_row(cnt, k, B, gap):
    """A row whose k winners are exactly the elements >= 1/2 at indices <= B (and, if k > B + 1, 1.0s further on), the last
    of them a 1/2 at index B; one more 1/2 follows at index B + 1 (gap False) or B + GAP (gap True) and must lose.
    Everything else is 1/4."""
    nxt = B + (GAP if gap else 1)
    assert 1 <= k < cnt and nxt < cnt
    v = np.full(cnt, 0.25, dtype=np.float32)
    inside = min(k, B + 1)
    rs = np.random.RandomState(B * 2 + gap)
    taken = np.concatenate([rs.choice(B, inside - 1, replace=False), [B]]).astype(np.int64) if inside > 1 else np.array([B])
    v[taken] = np.where(rs.rand(taken.size) < 0.5, 1.0, 0.5)
    v[B] = 0.5
    v[nxt] = 0.5
    extra = k - inside
    if extra:
        free = np.setdiff1d(np.arange(B + 1, cnt), [nxt])
        v[free[:: max(1, free.size // extra)][:extra]] = 1.0
    return v


def boundary_levels():
    """(cnt, k, B, gap) for every boundary, the next equal directly behind it and a sweep away, with k = B + 1 (every
    element up to B wins) where 2048 allows and with a k that leaves losers below B."""
    out = []
    for B in BOUNDARIES:
        for gap in (False, True):
            cnt = B + (GAP if gap else 1) + 3
            for k in sorted({min(B + 1, MAX_K), min(max(B // 2, 1), 1000)}):
                out.append((cnt, k, B, gap))
    return out


# ========================================================================== detections: exactly known scores and boxes

C91 = 91
HOT, COLD = 40.0, -40.0
SCORE_THRESH, DET_MIN_SIZE, DET_NMS, DET_D = 0.05, 1e-2, 0.5, 100
BOX_WEIGHTS = (10.0, 10.0, 5.0, 5.0)
AT_THR2 = 2 * AT_THR                 # even sides: intersection 16, union 32: IoU exactly 0.5, not suppressed


def saturated_logits(hot, C=C91):
    """hot: per RoI the list of its hot classes, m in {1, 2, 4, 8, 16, 32} of them (1 .. C - 1).  +40 there, -40 everywhere
    else, background included: the softmax is exactly 1 / m on the hot classes (and ~ e^-80 elsewhere)."""
    lg = np.full((len(hot), C), COLD, dtype=np.float32)
    for r, cs in enumerate(hot):
        assert len(cs) in (1, 2, 4, 8, 16, 32) and len(set(cs)) == len(cs) and all(1 <= c < C for c in cs)
        lg[r, list(cs)] = HOT
    return lg


def _spread(first, m):
    """m distinct classes starting at `first`, stepping by 7 (wrapping inside 1 .. 90; 7 and 90 share no factor)."""
    return [1 + (first - 1 + 7 * i) % (C91 - 1) for i in range(m)]


def _even_grid(n, x0=0, y0=100):
    """n disjoint 4 x 4 boxes, pitch 6."""
    return _grid_boxes(n, size=4, pitch=6, per_row=100, x0=x0, y0=y0)


def det_case(name, R):
    """One image's head outputs: dict(logits [R, 91], deltas [R, 364], rois [R, 4], shape (h, w), hot).  Zero deltas except
    where a case says otherwise: every class's box is the RoI itself.

      saturated   disjoint boxes, every RoI one hot class (score exactly 1.0): classes 5 and 2 take n1 = min(40, R // 3)
                  RoIs each, class 60 the rest -- for R = 1000 more than D survivors, all tied, 920 of them in one class:
                  (class, rank) alone decides who is reported and with which label;
      mixed       suppressing pairs, an exact-threshold pair, duplicates (in one class and across two), a zero-width RoI, a
                  NaN delta row, a chain whose members tie, then disjoint boxes with 1 / m scores, m = 32 (dropped) among them;
      dropped     every row has 32 hot classes: 1 / 32 <= score_thresh, nothing is left;
      orderfree   disjoint or identical boxes only, fewer than D survivors: the result is the same multiset whatever
                  order ties are taken in."""
    hot, rois = [], []
    deltas = np.zeros((R, 4 * C91), dtype=np.float32)
    if name == "saturated":
        n1 = min(40, R // 3)
        hot = [[5] if i < n1 else ([2] if i < 2 * n1 else [60]) for i in range(R)]
        rois = _even_grid(R)
    elif name == "dropped":
        hot = [_spread(1 + i % 7, 32) for i in range(R)]
        rois = _even_grid(R)
    elif name == "orderfree":
        rois = _even_grid(R)
        for i in range(R):
            hot.append(_spread(1 + i % 11, (1, 2, 4, 1, 8)[i % 5]) if i < 30 else _spread(1 + i % 7, 32))
        rois[1::4][:6] = rois[0::4][:6]                                          # identical boxes with overlapping class sets
    elif name == "mixed":
        special = [
            (ABOVE_THR[0], [9]), (ABOVE_THR[1], [9]),                              # 70 / 130: the second is suppressed (lower index first)
            (_even_grid(1, x0=200, y0=0)[0], [9, 12]), (_even_grid(1, x0=200, y0=0)[0], [12, 9]),   # duplicates at 1 / 2 in two classes
            (np.array([300, 0, 300, 10]), [9]),                                    # zero width: dropped by size
            (np.array([320, 0, 330, 10]), [9]),                                    # its class-9 deltas are NaN: dropped
            (AT_THR2[0] + [400, 0, 400, 0], [9]), (AT_THR2[1] + [400, 0, 400, 0], [9]),              # IoU 0.5 exactly: both stay
            (_even_grid(1, x0=500, y0=0)[0], [9]), (_even_grid(1, x0=500, y0=0)[0], [9]),           # duplicates in one class: one stays
        ]
        chain = [(b + [0, 40, 0, 40], [20, 30]) for b in _chain(12)]                # tied at 1 / 2 in two classes: 0, 2, 4, .. stay
        rows = (special + chain)[:R]
        grid = _even_grid(max(R - len(rows), 0))
        rows += [(grid[i], _spread(1 + i % 13, (1, 2, 4, 8, 16, 32)[i % 6])) for i in range(len(grid))]
        rois, hot = np.stack([r for r, _ in rows]), [h for _, h in rows]
        if R > 5:
            deltas[5, 4 * 9:4 * 9 + 4] = np.nan
    else:
        raise KeyError(name)
    rois = np.asarray(rois, dtype=np.float32)
    assert rois.shape == (R, 4) and len(hot) == R
    return dict(logits=saturated_logits(hot), deltas=deltas, rois=rois, shape=(800, 1333), hot=hot)


def det_inputs_cpu(case):
    """(scores [R, C], boxes [R, C, 4]) of a case as the CPU tensor path computes them, with the generators' two
    preconditions asserted: the softmax is exactly 1 / m on the hot classes and at most e^-79 elsewhere, and every box
    without a NaN delta decodes to its (integer, even-sided) RoI."""
    lg, dl, rois = torch.tensor(case["logits"]), torch.tensor(case["deltas"]), torch.tensor(case["rois"])
    scores = F.softmax(lg, -1)
    check_exact_scores(scores.numpy(), case["hot"])
    boxes = ops.clip_boxes_to_image(ops.BoxCoder(BOX_WEIGHTS).decode(dl, rois), case["shape"])
    r = case["rois"]
    assert np.array_equal(r, np.rint(r)) and not ((r[:, 2:] - r[:, :2]) % 2).any() and (r >= 0).all()
    assert (r[:, 2] <= case["shape"][1]).all() and (r[:, 3] <= case["shape"][0]).all()
    nan = torch.tensor(case["deltas"]).view(len(r), -1, 4).isnan().any(-1)
    want = rois[:, None, :].expand(-1, lg.shape[1], -1)
    assert torch.equal(boxes[~nan], want[~nan]) and boxes[nan].isnan().all()
    return scores.numpy(), boxes.numpy()


def check_exact_scores(scores, hot):
    """scores [R, C] (background first): exactly 1 / m on the hot classes, nothing above e^-79 elsewhere."""
    for r, cs in enumerate(hot):
        row = scores[r].copy()
        assert (row[list(cs)] == np.float32(1.0 / len(cs))).all(), (r, cs, row[list(cs)])
        row[list(cs)] = 0
        assert (row <= 1e-34).all() and (row >= 0).all()


def det_ref(case, D=DET_D):
    scores, boxes = det_inputs_cpu(case)
    return detections_ref(scores, boxes, SCORE_THRESH, DET_MIN_SIZE, DET_NMS, D)


def bare_roi_heads(D=DET_D):
    """RoIHeads with the reference's post-processing settings and no networks attached."""
    return RoIHeads(None, None, None, 0.5, 0.5, 512, 0.25, None, SCORE_THRESH, DET_NMS, D)


def as_multiset(boxes, labels, scores):
    return sorted((int(l), tuple(float(x) for x in b), float(s)) for b, l, s in zip(np.asarray(boxes), np.asarray(labels), np.asarray(scores)))


# ======================================================================================== RPN filter: tied objectness

RPN_PRE = RPN_POST = dict(training=2000, testing=1000)
RPN_NMS, RPN_MIN_SIZE = 0.7, 1e-3
RPN_COUNTS = ([16385, 300, 75, 20, 5], [40000, 17000, 9], [50, 30, 20, 10, 5])
RPN_SIZES = ((1333.0, 800.0), (1200.0, 704.0))          # (w, h) of the two images


def bare_rpn():
    return RegionProposalNetwork(None, None, 0.7, 0.3, 256, 0.5, RPN_PRE, RPN_POST, RPN_NMS)


def rpn_case(counts, seed, tied=True):
    """(proposals [2, A, 4], objectness [2, A], sizes [2, 2]) as CPU tensors.  Objectness on the grid of 1/4 in [-2, 2]
    (tied = False: distinct values); integer proposals, corners from 60 outside the image on, sides 0 .. 300, every 7th a
    sliver of zero width, some wholly outside the image (clipped to nothing)."""
    rs = np.random.RandomState(seed)
    A, N = sum(counts), 2
    if tied:
        obj = rs.randint(-8, 9, (N, A)) / 4.0
    else:
        obj = np.stack([rs.permutation(A) for _ in range(N)]) / 64.0 - A / 128.0
    xy = np.stack([rs.randint(-60, 1400, (N, A)), rs.randint(-60, 860, (N, A))], -1)
    wh = rs.randint(0, 301, (N, A, 2))
    wh[:, ::7, 0] = 0
    props = np.concatenate([xy, xy + wh], -1)
    return torch.tensor(props.astype(np.float32)), torch.tensor(obj.astype(np.float32)), torch.tensor(RPN_SIZES)


# ================================================================================================================ CPU

def _eq(a, b):
    """bit-for-bit up to the payload of NaNs (both NaN, or equal with equal sign)"""
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(0.0, 1e30, -1e30), b.nan_to_num(0.0, 1e30, -1e30)) \
        and torch.equal(torch.signbit(a) | a.isnan(), torch.signbit(b) | b.isnan())


def test_stable_sort_orders_nan_zeros_and_denormals_as_the_reference_needs():
    """One hand-written vector with everything in it: NaN first (both of them, in index order), +inf, numbers, the
    denormal 1e-45 above the zeros, +0 and -0 in index order, -1e-45 below them, -inf last."""
    tiny = 2.0 ** -149
    v = torch.tensor([0.0, -tiny, float("nan"), -0.0, 1.0, tiny, NEG_INF, 0.0, float("inf"), -0.0, float("nan"), 1.0, -1.0])
    assert float(v[5]) == float(torch.tensor(1e-45)) and float(v[5]) > 0.0 > float(v[1]) == float(torch.tensor(-1e-45))
    s, i = torch.sort(v, descending=True, stable=True)
    assert i.tolist() == [2, 10, 8, 4, 11, 5, 0, 3, 7, 9, 1, 12, 6]
    assert torch.signbit(s[6:10]).tolist() == [False, True, False, True]
    ts, ti, _, _ = topk_stable(v[None], [13], [13], 14)
    assert ti[0, 0].tolist() == [2, 10, 8, 4, 11, 5, 0, 3, 7, 9, 1, 12, 6, 0] and float(ts[0, 0, 13]) == NEG_INF and _eq(ts[0, 0, :13], s)
    assert topk_key(v.numpy())[[0, 3]].tolist() == [0x80000000] * 2 and topk_key(v.numpy())[5] == 0x80000001 and topk_key(v.numpy())[1] == 0x7ffffffe
    assert np.array_equal(np.argsort(-topk_key(v.numpy()).astype(np.int64), kind="stable"), i.numpy())


def test_topk_stable_levels_padding_boxes_and_offset():
    """Two rows, three levels (one empty), hand-computed; boxes gathered, clipped and flagged; columns outside the levels
    (offset0) never looked at."""
    v = torch.tensor([[9.0, 9.0, 1.0, 2.0, 2.0, 5.0, 5.0, 9.0],
                      [9.0, 9.0, 3.0, 3.0, NEG_INF, 4.0, 9.0, 9.0]])
    boxes = torch.zeros(2, 8, 4)
    boxes[:, :, 2:] = torch.arange(8.0)[None, :, None] + 1                  # box a = [0, 0, a + 1, a + 1]
    boxes[0, 4] = torch.tensor([-3.0, 2.0, 9.0, 2.0])                       # clipped to [0, 2, 6, 2]: zero height
    s, ix, b, ok = topk_stable(v, [3, 0, 2], [2, 1, 2], 3, boxes, torch.tensor([[6.0, 5.0], [4.0, 4.0]]), 1.0, offset0=2)
    assert s.tolist() == [[[2.0, 2.0, NEG_INF], [NEG_INF] * 3, [5.0, 5.0, NEG_INF]], [[3.0, 3.0, NEG_INF], [NEG_INF] * 3, [9.0, 4.0, NEG_INF]]]
    assert ix.tolist() == [[[1, 2, 0], [0, 0, 0], [0, 1, 0]], [[0, 1, 0], [0, 0, 0], [1, 0, 0]]]
    assert b[0, 0].tolist() == [[0, 0, 4, 4], [0, 2, 6, 2], [0, 0, 0, 0]] and b[0, 2].tolist() == [[0, 0, 6, 5], [0, 0, 6, 5], [0, 0, 0, 0]]
    assert b[1, 2].tolist() == [[0, 0, 4, 4], [0, 0, 4, 4], [0, 0, 0, 0]]
    assert ok.tolist() == [[[True, False, False], [False] * 3, [True, True, False]], [[True, True, False], [False] * 3, [True, True, False]]]
    s2, ix2, b2, ok2 = topk_stable(v[1:], [3], [3], 3, boxes[1:], None, 0.0, offset0=2)          # a -inf winner: gathered, not valid
    assert ix2.tolist() == [[[0, 1, 2]]] and b2[0, 0, 2].tolist() == [0, 0, 5, 5] and ok2.tolist() == [[[True, True, False]]]


def test_detections_ref_by_hand_two_classes_five_rois():
    """C = 3 (background, classes 1 and 2), D = 10, score_thresh 0.05, min_size 0.01, NMS at 0.5.

        r0 [0, 0, 10, 10]    r1 [3, 0, 13, 10]  (IoU 7 / 13 with r0)    r2 = r3 = [20, 0, 30, 10]    r4 [40, 0, 40, 10]  (zero width)
        class 1 scores  0.5  1.0  0.5   0.5  1.0        class 2 scores  1.0  0.03  0.25  1.0  0.5

    class 1: r4 dropped (size).  Order r1 (1.0), r0, r2, r3 (0.5, by index).  r1 removes r0, r2 removes its duplicate r3:
             r1 (1.0), r2 (0.5).
    class 2: r1 dropped (0.03 <= 0.05), r4 dropped (size).  Order r0, r3 (1.0, by index), r2 (0.25).  r3 removes r2: r0, r3.
    class-major (1, r1, 1.0) (1, r2, 0.5) (2, r0, 1.0) (2, r3, 1.0); the stable sort by score moves (1, r2) to the end and
    leaves the three 1.0 in (class, rank) order."""
    rois = np.array([[0, 0, 10, 10], [3, 0, 13, 10], [20, 0, 30, 10], [20, 0, 30, 10], [40, 0, 40, 10]], dtype=np.float32)
    scores = np.array([[0, 0.5, 1.0], [0, 1.0, 0.03], [0, 0.5, 0.25], [0, 0.5, 1.0], [0, 1.0, 0.5]], dtype=np.float32)
    boxes = np.repeat(rois[:, None], 3, axis=1)
    b, l, s, n = detections_ref(scores, boxes, 0.05, 0.01, 0.5, 10)
    assert n == 4 and l.tolist() == [1, 2, 2, 1] and s.tolist() == [1.0, 1.0, 1.0, 0.5]
    assert b.tolist() == [rois[1].tolist(), rois[0].tolist(), rois[3].tolist(), rois[2].tolist()]
    assert l.dtype == np.int64 and s.dtype == b.dtype == np.float32
    # background never reported, however high its score; a NaN box is dropped, not passed to the NMS
    scores[:, 0] = 1.0
    boxes[3, 2] = np.nan
    b, l, s, n = detections_ref(scores, boxes, 0.05, 0.01, 0.5, 10)
    assert n == 4 and l.tolist() == [1, 2, 1, 2] and s.tolist() == [1.0, 1.0, 0.5, 0.25] and b[3].tolist() == rois[2].tolist()


def test_detections_ref_by_hand_cut_inside_a_run_spanning_two_classes():
    """Four disjoint RoIs, D = 3 (d = 3).  Class 1 has r0 and r2 at 1.0, class 2 has r0, r1 and r3 at 1.0: five survivors,
    all tied, class-major (1, r0) (1, r2) (2, r0) (2, r1) (2, r3).  The cut keeps the first three: both of class 1 and
    only r0 of class 2.  With D = 2 per-class lists are cut to d = 2 first: (1, r0) (1, r2)."""
    rois = _even_grid(4).astype(np.float32)
    scores = np.array([[0, 1, 1], [0, 0, 1], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
    boxes = np.repeat(rois[:, None], 3, axis=1)
    b, l, s, n = detections_ref(scores, boxes, 0.05, 0.01, 0.5, 3)
    assert n == 3 and l.tolist() == [1, 1, 2] and s.tolist() == [1.0] * 3 and b.tolist() == rois[[0, 2, 0]].tolist()
    b, l, s, n = detections_ref(scores, boxes, 0.05, 0.01, 0.5, 2)
    assert n == 2 and l.tolist() == [1, 1] and b.tolist() == rois[[0, 2]].tolist()
    b, l, s, n = detections_ref(scores, boxes, 0.05, 0.01, 0.5, 100)
    assert n == 5 and l.tolist() == [1, 1, 2, 2, 2] and b.tolist() == rois[[0, 2, 0, 1, 3]].tolist()


def _dense_even(n, seed):
    """Clustered integer boxes with even sides inside 200 x 200: many pairs above IoU 0.5."""
    rs = np.random.RandomState(seed)
    c = rs.randint(0, 40, (n, 2)) * 2
    return np.concatenate([c, c + rs.randint(20, 32, (n, 2)) * 2], 1).astype(np.float32)


def test_detections_ref_equals_the_cpu_tensor_path_without_ties():
    heads = bare_roi_heads()
    for R, seed in ((300, 1), (37, 2), (1, 3)):
        g = torch.Generator().manual_seed(seed)
        logits = torch.randn(R, C91, generator=g) * 3
        rois = torch.tensor(_dense_even(R, seed))
        deltas = torch.zeros(R, 4 * C91)
        scores = F.softmax(logits, -1)
        live = scores[:, 1:][scores[:, 1:] > SCORE_THRESH]
        assert live.numel() > R // 2 and live.unique().numel() == live.numel()          # no ties among the candidates
        boxes = ops.clip_boxes_to_image(heads.box_coder.decode(deltas, rois), (800, 1333))
        assert torch.equal(boxes, rois[:, None, :].expand(-1, C91, -1))
        want = heads.postprocess_detections(logits, deltas, [rois], [(800, 1333)])[0]
        b, l, s, n = detections_ref(scores.numpy(), boxes.numpy(), SCORE_THRESH, DET_MIN_SIZE, DET_NMS, DET_D)
        assert n == want["scores"].numel() and (R < 37 or n >= 30)
        assert np.array_equal(s, want["scores"].numpy()) and np.array_equal(l, want["labels"].numpy()) and np.array_equal(b, want["boxes"].numpy())
        if R == 300:          # the NMS took part: fewer survivors than candidates in some class
            cand = (scores[:, 1:] > SCORE_THRESH).sum().item()
            assert detections_ref(scores.numpy(), boxes.numpy(), SCORE_THRESH, DET_MIN_SIZE, DET_NMS, 10 ** 6)[3] < cand


def test_rpn_filter_ref_equals_the_cpu_tensor_path_without_ties():
    rpn = bare_rpn()
    for counts, seed in (([3000, 300, 75, 20, 5], 1), ([2500, 1100, 9], 2)):
        props, obj, sizes = rpn_case(counts, seed, tied=False)
        assert all(o.unique().numel() == o.numel() for o in obj)
        for training in (True, False):
            rpn.train(training)
            boxes, scores, count = rpn._filter(props, obj.reshape(-1, 1), sizes, counts)
            want = rpn_filter_ref(props, obj, sizes, counts, rpn._n(RPN_PRE), rpn._n(RPN_POST), RPN_MIN_SIZE, RPN_NMS)
            for n, (wb, ws, wc) in enumerate(want):
                assert int(count[n]) == wc > 500
                assert np.array_equal(scores[n, :wc].numpy(), ws) and np.array_equal(boxes[n, :wc].numpy(), wb)
                assert (scores[n, wc:] == NEG_INF).all()
            full = rpn_filter_ref(props, obj, sizes, counts, rpn._n(RPN_PRE), rpn._n(RPN_POST), RPN_MIN_SIZE, RPN_NMS, with_all=True)
            valid = topk_stable(obj, counts, [min(rpn._n(RPN_PRE), c) for c in counts], max(min(rpn._n(RPN_PRE), c) for c in counts), props, sizes, RPN_MIN_SIZE)[3]
            assert all(f[1].size < int(valid[n].sum()) for n, f in enumerate(full))       # the NMS removed something
            assert not bool(valid.all())                                                     # and the size test did


def test_topk_families_have_the_structure_their_names_claim():
    seen = dict.fromkeys(("inside", "last", "first", "ordered", "inf_taken", "nan_won", "zero_tie_at_k"), 0)
    launches = geometry_launches()
    assert sorted((c, k) for cs, ks, _ in launches for c, k in zip(cs, ks)) == sorted(geometry_pairs())
    assert all(len(cs) <= MAX_LEVELS and max(Ks) <= MAX_K and Ks[0] == max(max(ks), 1) for cs, ks, Ks in launches)
    assert any(len(cs) == MAX_LEVELS for cs, _, _ in launches) and any(len(Ks) == 2 for _, _, Ks in launches)
    assert {c for c, _ in geometry_pairs()} == set(LENGTHS) and max(LENGTHS) == 16385
    for c in LENGTHS:
        have = {k for cc, k in geometry_pairs() if cc == c}
        assert have == {k for k in set(KS) | {c - 1, c} if 0 <= k <= min(c, MAX_K)} and 0 in have and min(c, MAX_K) in have
    for li, (counts, ks, _) in enumerate(launches):
        rows = family_rows(counts, ks, li)
        assert rows.shape == (len(FAMILIES), sum(counts)) and rows.dtype == np.float32
        off = 0
        for c, k in zip(counts, ks):
            lev = {name: rows[f, off:off + c] for f, name in enumerate(FAMILY_NAMES)}
            off += c
            for name, sign in (("near_one", 1), ("near_one_negated", -1)):
                v = lev[name]
                below = np.abs(v) < 1
                assert (np.abs(v) <= 1).all() and (np.abs(v) > 1 - 2.0 ** -14).all() and (np.sign(v) == sign).all()
                assert np.unique(topk_key(v[below]) >> 10).size <= 1                       # the upper 22 bits are shared
                if below.any() and (~below).any():
                    assert (topk_key(v[~below]) >> 21)[0] != (topk_key(v[below]) >> 21)[0]   # 1.0 itself: another first-pass bin
            for name in ("middle", "middle_negated"):
                v = lev[name][np.abs(lev[name]) < 1]
                assert np.unique(topk_key(v) >> 21).size <= 1 and (c < 64 or np.unique((topk_key(v) >> 10) & 0x7ff).size > 8)
                assert not (topk_key(v) & 0x3ff).any() or name == "middle_negated"
            v = lev["denormal"]
            assert (np.abs(v) < 2.0 ** -140).all() and np.array_equal(topk_key(v) == 0x80000000, v == 0)      # no denormal shares the zeros' key
            if denormal_room(c, k):
                first, last = kth_run(v, k)
                zero = np.flatnonzero(v == 0)
                assert first == k - 1 < last and np.signbit(v[zero]).any() and not np.signbit(v[zero]).all()
                assert (v > 0).sum() == k - 1 and (v < 0).sum() == c - k - (last - first)
                seen["zero_tie_at_k"] += 1
            for mode in ("inside", "last", "first"):
                v = lev["saturated_" + mode]
                assert np.isin(v, SAT_VALUES).all()
                if saturated_room(c, k, mode):
                    first, last = kth_run(v, k)
                    assert {"inside": first < k - 1 < last, "last": first < k - 1 == last, "first": first == k - 1 < last}[mode], (c, k, mode)
                    seen[mode] += 1
                    seen["ordered"] += int(last > k - 1)
            v = lev["inf_majority"]
            assert np.isfinite(v).sum() == min(5, c) and (v[~np.isfinite(v)] == NEG_INF).all()
            seen["inf_taken"] += int(k > 5)
            v = lev["nan"]
            assert np.isnan(v).sum() == min(3, c // 2) and (c < 64 or np.unique(v[~np.isnan(v)]).size <= 9)
            seen["nan_won"] += int(k >= 1 and np.isnan(v).any())
            assert (lev["constant"] == 0.25).all()
    assert all(v > 0 for v in seen.values()), seen
    assert seen["inside"] >= 60 and seen["last"] >= 60 and seen["first"] >= 60, seen


def test_boundary_rows_have_the_structure_their_names_claim():
    levels = boundary_levels()
    assert {(B, gap) for _, _, B, gap in levels} == {(B, g) for B in BOUNDARIES for g in (False, True)} and len(levels) <= MAX_LEVELS
    for cnt, k, B, gap in levels:
        v = boundary_row(cnt, k, B, gap)
        s, i = torch.sort(torch.tensor(v), descending=True, stable=True)
        taken = i[:k].numpy()
        eq = np.flatnonzero(v == 0.5)
        assert float(s[k - 1]) == 0.5 == float(s[k])                                     # the cut falls inside the run of 1/2
        assert int(i[k - 1]) == B == eq[np.isin(eq, taken)].max()                        # its last taken element sits on the boundary
        nxt = eq[eq > B].min()
        assert nxt == int(i[k]) and (nxt - B > 8192 if gap else nxt == B + 1)            # the next equal: directly behind, or a sweep away
        assert k <= MAX_K and (k == min(B + 1, MAX_K) or (v[:B] == 0.25).any())


def test_detection_cases_have_the_structure_their_names_claim():
    D = DET_D
    b, l, s, n = det_ref(det_case("saturated", 1000))
    full = det_ref(det_case("saturated", 1000), D=10 ** 6)
    assert n == D and (s == 1.0).all() and l.tolist() == [2] * 40 + [5] * 40 + [60] * 20            # (class, rank) decides the labels
    assert full[3] == 1000 and (full[2] == 1.0).all() and (full[1] == 60).sum() == 920 > min(D, 1000)      # more survivors than D, all at 1.0; a class above d
    grid = _even_grid(1000).astype(np.float32)
    assert np.array_equal(b, np.concatenate([grid[40:80], grid[:40], grid[80:100]]))                # lowest RoI index first within a class
    b, l, s, n = det_ref(det_case("saturated", 100))
    assert n == 100 == det_ref(det_case("saturated", 100), D=10 ** 6)[3] and l.tolist() == [2] * 33 + [5] * 33 + [60] * 34      # the run ends exactly at D
    b, l, s, n = det_ref(det_case("saturated", 101))
    assert n == 100 and det_ref(det_case("saturated", 101), D=10 ** 6)[3] == 101 and l.tolist() == [2] * 33 + [5] * 33 + [60] * 34
    assert np.array_equal(b[-1], _even_grid(101)[99])                                               # RoI 100 is the one that is cut
    for R in (7, 1):
        b, l, s, n = det_ref(det_case("saturated", R))
        assert n == R < D and (s == 1.0).all() and sorted(l.tolist()) == l.tolist()
    for R in (1, 7, 100, 101, 1000):
        assert det_ref(det_case("dropped", R))[3] == 0
        case = det_case("orderfree", R)
        b, l, s, n = det_ref(case)
        assert 0 < n < D and n == det_ref(case, D=10 ** 6)[3]
        ub = np.unique(b, axis=0)
        iw = np.minimum(ub[:, None, 2], ub[None, :, 2]) - np.maximum(ub[:, None, 0], ub[None, :, 0])
        ih = np.minimum(ub[:, None, 3], ub[None, :, 3]) - np.maximum(ub[:, None, 1], ub[None, :, 1])
        assert not ((iw > 0) & (ih > 0) & ~np.eye(len(ub), dtype=bool)).any()                       # disjoint or identical
        assert R < 7 or (np.unique(s).size < n and len(ub) < np.unique(case["rois"], axis=0).shape[0] + 1)
        case = det_case("mixed", R)
        b, l, s, n = det_ref(case)
        assert n > 0 and np.unique(s).size < max(n, 2)
    # mixed, spelled out for R = 100: class 9 keeps ABOVE_THR[0], one of the duplicates at 1/2 ... and the chain its even members
    case = det_case("mixed", 100)
    b, l, s, n = det_ref(case, D=10 ** 6)
    got = as_multiset(b, l, s)
    r = case["rois"]
    assert (9, tuple(r[0]), 1.0) in got and (9, tuple(r[1]), 1.0) not in got                        # 70 / 130 suppressed
    assert (9, tuple(r[6]), 1.0) in got and (9, tuple(r[7]), 1.0) in got                            # IoU 0.5 exactly: both stay
    assert got.count((9, tuple(r[2]), 0.5)) == 1 and got.count((12, tuple(r[2]), 0.5)) == 1         # duplicates: one per class
    assert got.count((9, tuple(r[8]), 1.0)) == 1
    assert not any(t[1] in (tuple(r[4]), tuple(r[5])) for t in got)                                 # zero width, NaN deltas
    for c in (20, 30):
        assert [t[1] for t in got if t[0] == c and t[1][1] == 40.0] == [tuple(r[10 + j]) for j in range(0, 12, 2)]
    assert not any(t[2] == np.float32(1 / 32) for t in got) and any(t[2] == np.float32(1 / 16) for t in got)
    assert n > DET_D and det_ref(case)[3] == DET_D
    first, last = kth_run(-np.sort(-s), DET_D)
    assert first <= DET_D - 1 < last                                     # the cut at D falls inside a run
    # every NMS decision of every case is made on integers below 2^24 after the move by class * (largest coordinate + 1)
    for name in ("saturated", "mixed", "orderfree", "dropped"):
        assert (C91 - 1) * (det_case(name, 1000)["rois"].max() + 1) + det_case(name, 1000)["rois"].max() < 2 ** 24


def test_rpn_cases_have_the_structure_their_names_claim():
    rpn = bare_rpn()
    inside_level = inside_final = 0
    for ci, counts in enumerate(RPN_COUNTS):
        props, obj, sizes = rpn_case(counts, 10 + ci)
        assert np.array_equal(obj.numpy() * 4, np.rint(obj.numpy() * 4)) and float(obj.min()) == -2 and float(obj.max()) == 2
        assert np.array_equal(props.numpy(), np.rint(props.numpy()))
        assert (props[..., 2] > sizes[:, None, 0]).any() and (props[..., 0] < 0).any() and (props[..., 2] == props[..., 0]).any()
        for training in (True, False):
            rpn.train(training)
            pre, post = rpn._n(RPN_PRE), rpn._n(RPN_POST)
            for n in range(2):
                if counts[0] > pre:
                    first, last = kth_run(obj[n, :counts[0]].numpy(), pre)
                    assert first < pre - 1 < last
                    inside_level += 1
            full = rpn_filter_ref(props, obj, sizes, counts, pre, post, RPN_MIN_SIZE, RPN_NMS, with_all=True)
            for _, s, count in full:
                assert count > 0 and np.unique(s).size <= 17
                if s.size > post:
                    assert count == post and s[post - 1] == s[post]
                    inside_final += 1
                else:
                    assert count == s.size
    assert inside_level >= 6 and inside_final >= 4, (inside_level, inside_final)
