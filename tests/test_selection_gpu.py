"""csrc/dib_topk.hip and its call sites on tied, saturated scores, bit for bit against the exact references of
tests/test_selection_reference.py (which asserts, on the CPU, that the references are right and that every generated
input has the ties its name claims).

  a. dib_topk_levels across key space (scores that share their upper key bits, denormals and zeros, runs of equal
     scores across the k-th place, -inf majorities, NaN) and geometry (row lengths and k around 64, 1024, 2048, 8192;
     k = 0 and k = cnt; empty levels; 32 levels; the raw entry point with columns outside every level);
  b. topk_levels_split_hip (long levels in pieces) on the same kinds of scores;
  c. RoIHeads.postprocess_detections / _detections_hip on softmax scores that are exactly 1 / m over integer boxes;
  d. RegionProposalNetwork._filter on objectness on a grid of 1/4 over integer proposals.

No tolerance appears: every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

from detectinblur_amd import _lib
from detectinblur_amd.models import detector_ops as ops
from tests import test_selection_reference as S
from tests.test_selection_reference import NEG_INF, _eq, topk_stable

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.uint8).cpu()


def _check_topk(values, counts, ks, K, boxes=None, clip_wh=None, min_size=0.0, rows=None):
    """One launch (twice: the bytes must not differ) against topk_stable: scores, indices, boxes, valid flags."""
    got, again = [ops.topk_levels_hip(values.cuda(), counts, ks, K, None if boxes is None else boxes.cuda(),
                                      None if clip_wh is None else clip_wh.cuda(), min_size, want_index=True) for _ in range(2)]
    ws, wi, wb, wv = topk_stable(values, counts, ks, K, boxes, clip_wh, min_size)
    names = rows or list(range(values.shape[0]))
    s, ix = got[0].cpu(), got[1].cpu()
    for n, name in enumerate(names):
        for l in range(len(counts)):
            where = (name, "level", l, "cnt", counts[l], "k", ks[l], "K", K)
            assert _eq(s[n, l], ws[n, l]), ("scores",) + where
            assert torch.equal(ix[n, l], wi[n, l]), ("index",) + where + (ix[n, l][ix[n, l] != wi[n, l]][:4].tolist(), wi[n, l][ix[n, l] != wi[n, l]][:4].tolist())
    if boxes is not None:
        assert got[3].dtype == torch.bool
        assert _eq(got[2].cpu(), wb) and torch.equal(got[3].cpu(), wv)
    for a, b in zip(got, again):
        assert (a is None and b is None) or torch.equal(_bits(a), _bits(b)), "two calls differ"
    return got


# ------------------------------------------------------------------------------------------ a. key space and geometry

@functools.lru_cache(maxsize=None)
def _launch_inputs(li):
    counts, ks, Ks = S.geometry_launches()[li]
    rows = torch.tensor(S.family_rows(counts, ks, li))
    return counts, ks, Ks, rows, S.index_boxes(rows.shape[0], rows.shape[1])


@pytest.mark.parametrize("li", range(len(S.geometry_launches())))
def test_families_at_every_row_length_and_k(li):
    """Every family as a row, every (row length, k) of a slice of the geometry as a level (up to 32 per launch), K = the
    largest k and K above it; boxes gathered, clipped and flagged by the same launch."""
    counts, ks, Ks, rows, boxes = _launch_inputs(li)
    clip = torch.tensor([S.CLIP_WH] * rows.shape[0])
    for K in Ks:
        _check_topk(rows, counts, ks, K, boxes, clip, 1.0, rows=S.FAMILY_NAMES)
    _check_topk(rows, counts, ks, Ks[-1])                      # scores and indices alone: no boxes, no clip


def test_ties_whose_last_winner_sits_on_a_wave_or_sweep_boundary():
    """Rows whose last equal-score winner has index 63, 64, 1023, 1024, 8191 or 8192, the first loser of the same score
    directly behind it or a whole unrolled sweep further on; a constant row of every such length."""
    levels = S.boundary_levels()
    counts, ks = [c for c, _, _, _ in levels], [k for _, k, _, _ in levels]
    rows = torch.tensor(np.stack([np.concatenate([S.boundary_row(*lv) for lv in levels]), np.full(sum(counts), 0.25, dtype=np.float32)]))
    boxes = S.index_boxes(2, rows.shape[1])
    got = _check_topk(rows, counts, ks, max(ks), boxes, None, 0.0, rows=["boundary", "constant"])
    ix = got[1].cpu()
    for l, (cnt, k, B, gap) in enumerate(levels):
        assert int(ix[0, l, :k].max()) >= B and B in ix[0, l, :k].tolist() and B + (S.GAP if gap else 1) not in ix[0, l, :k].tolist()
        assert ix[1, l, :k].tolist() == list(range(k))


def test_empty_levels_k_zero_and_32_levels():
    """An empty level between two live ones (asked for 0 and for 3 winners), k = 0 on a live level, 32 levels in one launch."""
    rs = np.random.RandomState(3)
    counts = [5, 0, 7, 0, 64, 1] + [3 + (i * 37) % 90 for i in range(26)]
    ks = [3, 0, 7, 3, 0, 1] + [(i * 5) % 9 for i in range(26)]
    assert len(counts) == ops.TOPK_MAX_LEVELS == S.MAX_LEVELS
    rows = torch.tensor(np.stack([S.SAT_VALUES[rs.randint(0, 5, sum(counts))], (rs.randint(-4, 5, sum(counts)) / 4.0).astype(np.float32)]))
    boxes = S.index_boxes(2, rows.shape[1])
    for K in (7, 8, 40):
        got = _check_topk(rows, counts, [min(k, K) for k in ks], K, boxes, torch.tensor([S.CLIP_WH] * 2), 1.0)
        assert (got[0][:, [1, 3, 4]] == NEG_INF).all() and not got[3][:, [1, 3, 4]].any() and not got[2][:, [1, 3, 4]].any()


FILL = {"s": 12345.0, "i": -99, "b": 12345.0, "v": 77}
BORDER = 256         # elements on either side of an output; 1 KiB of float32: the interior stays 16-byte aligned


def _bordered(shape, dtype, fill):
    """(flat buffer filled with `fill`, the view of its interior with `shape`)"""
    n = int(np.prod(shape))
    flat = torch.full((n + 2 * BORDER,), fill, dtype=dtype, device="cuda")
    return flat, flat[BORDER:BORDER + n].view(shape)


@pytest.mark.parametrize("want_index,want_boxes,want_clip", [(True, True, True), (False, True, False), (True, False, False), (False, False, False)])
def test_raw_entry_point_offset_stride_and_untouched_borders(want_index, want_boxes, want_clip):
    """dib_topk_levels itself: level_offset[0] = 5 and a row_stride seven past the last level -- the columns outside every
    level hold +inf and NaN and must never win --, N = 3, with and without out_index, boxes and clip_wh; the output
    buffers lie inside larger ones whose borders must come back untouched."""
    rs = np.random.RandomState(11)
    counts, ks, K, N = [70, 0, 1030, 9, 2049], [64, 0, 1025, 9, 1030], 1030, 3
    A = sum(counts)
    stride = 5 + A + 7
    body = np.stack([S.SAT_VALUES[rs.randint(0, 5, A)], S._fam_nan(A, 0, rs), S._fam_denormal(A, 0, rs)])
    values = torch.full((N, stride), float("inf"))
    values[:, 1:5:2] = float("nan"); values[:, stride - 7::2] = float("nan")
    values[:, 5:5 + A] = torch.tensor(body)
    assert values[:, :5].isnan().any() and values[:, :5].isinf().any() and values[:, -7:].isnan().any() and values[:, -7:].isinf().any()
    boxes = S.index_boxes(N, stride) if want_boxes else None
    clip = torch.tensor([S.CLIP_WH, (50.0, 40.0), (1000.0, 1000.0)]) if want_clip else None
    offs = [5]
    for c in counts:
        offs.append(offs[-1] + c)
    L = len(counts)
    v_dev = values.cuda()
    b_dev = boxes.cuda().contiguous() if want_boxes else None
    c_dev = clip.cuda() if want_clip else None
    assert b_dev is None or b_dev.data_ptr() % 16 == 0

    def call():
        bufs = {"s": _bordered((N, L, K), torch.float32, FILL["s"]), "i": _bordered((N, L, K), torch.int64, FILL["i"]) if want_index else None,
                "b": _bordered((N, L, K, 4), torch.float32, FILL["b"]) if want_boxes else None,
                "v": _bordered((N, L, K), torch.uint8, FILL["v"]) if want_boxes else None}
        ptr = {k: (x[1].data_ptr() if x is not None else None) for k, x in bufs.items()}
        assert ptr["b"] is None or ptr["b"] % 16 == 0
        _lib.check(_lib.lib().dib_topk_levels(v_dev.data_ptr(), stride, N, _lib.int_array(offs), _lib.int_array(ks), L, K,
                                              b_dev.data_ptr() if want_boxes else None, c_dev.data_ptr() if want_clip else None, 1.0,
                                              ptr["s"], ptr["i"], ptr["b"], ptr["v"], _lib.stream_of(v_dev)))
        for name, x in bufs.items():
            if x is not None:
                flat, inner = x
                assert (flat[:BORDER] == FILL[name]).all() and (flat[BORDER + inner.numel():] == FILL[name]).all(), "border of %s written" % name
        return [bufs[k][1].clone() if bufs[k] is not None else None for k in ("s", "i", "b", "v")]

    got, again = call(), call()
    ws, wi, wb, wv = topk_stable(values, counts, ks, K, boxes, clip, 1.0, offset0=5)
    assert _eq(got[0].cpu(), ws) and not got[0].isposinf().any()
    if want_index:
        assert torch.equal(got[1].cpu(), wi)
    if want_boxes:
        assert _eq(got[2].cpu(), wb) and torch.equal(got[3].cpu().bool(), wv) and int(got[3].max()) <= 1
    for a, b in zip(got, again):
        assert (a is None and b is None) or torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------- b. levels in pieces

@pytest.mark.parametrize("counts", [[16385, 300, 75, 20, 5], [40000, 17000, 9]])
def test_split_levels_equal_the_stable_sort(counts):
    """topk_levels_split_hip (the first level cut in pieces, merged by a second launch) on saturated and -inf-majority rows."""
    pieces = sum(max(1, -(-c // ops.TOPK_PIECE)) for c in counts)
    assert len(counts) < pieces <= ops.TOPK_MAX_LEVELS
    for K in (1000, 2000):
        ks = [min(K, c) for c in counts]
        rs = np.random.RandomState(K + len(counts))
        rows = [np.concatenate([S._fam_saturated(c, k, rs, mode) for c, k in zip(counts, ks)]) for mode in ("inside", "last", "first")]
        rows.append(np.concatenate([S._fam_inf_majority(c, k, rs) for c, k in zip(counts, ks)]))
        few = np.full(sum(counts), NEG_INF, dtype=np.float32)                 # finite scores in the LAST piece of the long level only
        few[counts[0] - 40:counts[0] - 1:3] = 0.5
        rows.append(few)
        values = torch.tensor(np.stack(rows))
        for mode, row in zip(("inside", "last", "first"), rows):
            first, last = S.kth_run(row[:counts[0]], ks[0])
            assert {"inside": first < K - 1 < last, "last": first < K - 1 == last, "first": first == K - 1 < last}[mode]
        assert np.isfinite(rows[3][:counts[0]]).sum() < K and 0 < np.isfinite(few[:counts[0]]).sum() < K
        N = values.shape[0]
        boxes = S.index_boxes(N, values.shape[1])
        clip = torch.tensor([S.CLIP_WH, (50.0, 40.0)] * 3)[:N]
        out = [ops.topk_levels_split_hip(values.cuda(), counts, ks, K, boxes.cuda(), clip.cuda(), 1.0) for _ in range(2)]
        ws, _, wb, wv = topk_stable(values, counts, ks, K, boxes, clip, 1.0)
        s, b, v = out[0]
        assert _eq(s.cpu(), ws) and torch.equal(v.cpu(), wv)
        assert _eq(b.cpu(), wb)
        for a, c in zip(out[0], out[1]):
            assert torch.equal(_bits(a), _bits(c))


# ------------------------------------------------------------------------------------------------------ c. detections

DET_R = (1, 7, 100, 101, 1000)


@functools.lru_cache(maxsize=None)
def _det(name, R):
    case = S.det_case(name, R)
    return case, S.det_inputs_cpu(case), S.det_ref(case)


def _cuda(case):
    return torch.tensor(case["logits"]).cuda(), torch.tensor(case["deltas"]).cuda(), torch.tensor(case["rois"]).cuda()


def _assert_detections(out, want, where):
    wb, wl, ws, n = want
    assert out["scores"].numel() == n, where + ("count", out["scores"].numel(), n)
    assert out["labels"].dtype == torch.int64 and out["boxes"].shape == (n, 4)
    assert np.array_equal(out["scores"].cpu().numpy(), ws), where + ("scores",)
    assert np.array_equal(out["labels"].cpu().numpy(), wl), where + ("labels", out["labels"].tolist(), wl.tolist())
    assert np.array_equal(out["boxes"].cpu().numpy(), wb), where + ("boxes",)


@pytest.mark.parametrize("R", DET_R)
@pytest.mark.parametrize("name", ["saturated", "mixed", "dropped", "orderfree"])
def test_detections_on_exact_tied_scores(name, R, monkeypatch):
    """postprocess_detections on the kernels and _detections_hip(defer=True) against detections_ref: the same boxes,
    labels and scores in the same order, the same count, -inf past it."""
    case, (scores, boxes), want = _det(name, R)
    heads = S.bare_roi_heads()
    logits, deltas, rois = _cuda(case)
    assert ops.hip_boxes_ok(logits, deltas, rois)
    # the generators' preconditions from the device's own candidates: scores exactly 1 / m, boxes the RoIs themselves
    s_cm, b_cm, stats = ops.det_candidates_hip(heads.box_coder, logits, deltas, rois, case["shape"], S.SCORE_THRESH, S.DET_MIN_SIZE)
    ok = (scores > S.SCORE_THRESH) & ((boxes[..., 2] - boxes[..., 0]) >= S.DET_MIN_SIZE) & ((boxes[..., 3] - boxes[..., 1]) >= S.DET_MIN_SIZE)
    ok = ok[:, 1:].T
    s_cm, b_cm = s_cm.cpu().numpy(), b_cm.cpu().numpy()
    assert np.array_equal(s_cm > NEG_INF, ok) and np.array_equal(s_cm[ok], scores[:, 1:].T[ok]) and int(stats[0]) == int(ok.sum())
    assert np.array_equal(b_cm[ok], np.transpose(boxes[:, 1:], (1, 0, 2))[ok])
    for r, cs in enumerate(case["hot"]):
        for c in cs:
            assert s_cm[c - 1, r] in (np.float32(1.0 / len(cs)), np.float32(NEG_INF))
    out = heads.postprocess_detections(logits, deltas, [rois], [case["shape"]])[0]
    _assert_detections(out, want, (name, R))
    tb, ts, tl, tn = heads._detections_hip(logits, deltas, rois, case["shape"], defer=True)
    n = int(tn)
    assert n == want[3] and tb.shape[0] == ts.shape[0] == tl.shape[0] == min(S.DET_D, (S.C91 - 1) * min(S.DET_D, R))
    _assert_detections({"boxes": tb[:n], "scores": ts[:n], "labels": tl[:n]}, want, (name, R, "deferred"))
    assert (ts[n:] == NEG_INF).all()
    if name in ("orderfree", "dropped"):          # the result does not depend on the order of ties: the tensor path agrees as a multiset
        monkeypatch.setattr(ops, "HIP_BOXES", False)
        ref = heads.postprocess_detections(logits, deltas, [rois], [case["shape"]])[0]
        assert S.as_multiset(ref["boxes"].cpu(), ref["labels"].cpu(), ref["scores"].cpu()) == S.as_multiset(*want[:3])


def test_detections_two_images_of_different_sizes_padded_path():
    """Two images in one call (101 saturated RoIs at 800 x 1333, 7 mixed ones at 600 x 900) through postprocess_detections
    and through padded_detections (the sync-free form), whose first n rows and n must equal the reference."""
    a, b = S.det_case("saturated", 101), dict(S.det_case("mixed", 7), shape=(600, 900))
    wants = [S.det_ref(a), S.det_ref(b)]
    heads = S.bare_roi_heads()
    la, da, ra = _cuda(a)
    lb, db, rb = _cuda(b)
    logits, deltas = torch.cat((la, lb)), torch.cat((da, db))
    out = heads.postprocess_detections(logits, deltas, [ra, rb], [a["shape"], b["shape"]])
    for i, (o, w) in enumerate(zip(out, wants)):
        _assert_detections(o, w, ("image", i))
    heads.box_roi_pool = lambda features, proposals, shapes: None
    heads.box_head = lambda x: x
    heads.box_predictor = lambda x: (logits, deltas)
    padded, rest = heads.padded_detections(None, [ra, rb], [a["shape"], b["shape"]])
    assert rest is None and len(padded) == 2
    for i, ((pb, ps, pl, pn), w) in enumerate(zip(padded, wants)):
        n = int(pn)
        _assert_detections({"boxes": pb[:n], "scores": ps[:n], "labels": pl[:n]}, w, ("padded image", i))
        assert (ps[n:] == NEG_INF).all()


# ------------------------------------------------------------------------------------------------------ d. RPN filter

@functools.lru_cache(maxsize=None)
def _rpn(ci, training):
    counts = S.RPN_COUNTS[ci]
    props, obj, sizes = S.rpn_case(counts, 10 + ci)
    key = "training" if training else "testing"
    return props, obj, sizes, S.rpn_filter_ref(props, obj, sizes, counts, S.RPN_PRE[key], S.RPN_POST[key], S.RPN_MIN_SIZE, S.RPN_NMS)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("ci", range(len(S.RPN_COUNTS)))
def test_rpn_filter_on_tied_objectness(ci, training):
    """rpn._filter (levels in pieces, NMS per level, last ranking) against rpn_filter_ref: count, boxes[:count] and
    scores[:count] exactly, -inf past the count; twice, the same bytes."""
    counts = S.RPN_COUNTS[ci]
    props, obj, sizes, want = _rpn(ci, training)
    rpn = S.bare_rpn()
    rpn.train(training)
    p, o, z = props.cuda(), obj.cuda().reshape(-1, 1), sizes.cuda()
    assert ops.hip_boxes_ok(o, p, z) and len(counts) <= 16
    out = [rpn._filter(p, o, z, counts) for _ in range(2)]
    boxes, scores, count = out[0]
    post = min(rpn._n(S.RPN_POST), len(counts) * max(min(rpn._n(S.RPN_PRE), c) for c in counts))
    assert boxes.shape == (2, post, 4) and scores.shape == (2, post)
    for n, (wb, ws, wc) in enumerate(want):
        assert int(count[n]) == wc, (n, int(count[n]), wc)
        assert np.array_equal(scores[n, :wc].cpu().numpy(), ws), (n, "scores")
        bad = np.flatnonzero((boxes[n, :wc].cpu().numpy() != wb).any(1))
        assert bad.size == 0, (n, "boxes", bad[:5].tolist(), ws[bad[:5]].tolist())
        assert (scores[n, wc:] == NEG_INF).all()
    for a, b in zip(out[0], out[1]):
        assert torch.equal(_bits(a), _bits(b))
