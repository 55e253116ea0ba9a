"""Detection overlays on the host (detectinblur_amd/overlay.py; reference engine.py:382-383, utils.py:279-353): the colours against the
reference's own, the outline rule of include/dib.h against pictures written out by hand, the pixel conversion, the files
`engine.evaluate(image_output_folder=...)` writes, the driver's --save_images, the C entry point's argument errors and the PNG writer.

tests/golden/overlay_colors.json was produced once, where the reference tree is mounted, by

    import json, torch, ref_harness                       # oracle/ref_harness.py: the reference's utils.py behind its import stubs
    colors = ref_harness.load().utils.compute_colors_for_labels(torch.arange(91)).tolist()
    byte = lambda c: min(max(int(round(c)), 0), 255)      # cv2's scalar -> uchar: round half to even (Python's round), saturate
    rgb = [byte(c[2]) | byte(c[1]) << 8 | byte(c[0]) << 16 for c in colors]      # (r, g, b) drawn into BGR, then BGR -> RGB
    json.dump({"colors": colors, "rgb": rgb}, open("tests/golden/overlay_colors.json", "w"), indent=0)
"""
import contextlib
import io
import json
import os
import threading

import numpy as np
import pytest
import torch

from detectinblur_amd import overlay, utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "overlay_colors.json")))
H, W = 12, 16


def background(h=H, w=W):
    """k / 255 with k = (7 x + 13 y + 50 c) % 256: float32(k / 255) * 255 truncates back to k (test_pixel_conversion pins that)"""
    c, y, x = np.meshgrid(np.arange(3), np.arange(h), np.arange(w), indexing="ij")
    k = (7 * x + 13 * y + 50 * c) % 256
    return torch.from_numpy((k / 255.0).astype(np.float32)), np.ascontiguousarray(k.transpose(1, 2, 0).astype(np.uint8))


def unpack(rgb):
    return [rgb & 255, rgb >> 8 & 255, rgb >> 16 & 255]


def expected(picture, legend):
    """`picture`: 12 strings of 16 characters, '.' = the background shows, any other character = the colour of label legend[ch]"""
    assert len(picture) == H and all(len(r) == W for r in picture), [len(r) for r in picture]
    _, want = background()
    for y, row in enumerate(picture):
        for x, ch in enumerate(row):
            if ch != ".":
                want[y, x] = unpack(GOLDEN["rgb"][legend[ch]])
    return want


# label 1 -> '#' / 'a', label 2 -> 'b'.  Every picture below is derived by hand from the rule in include/dib.h.
CASES = {
    # xa..xb = 4..11, ya..yb = 3..8: outer 3..12 x 2..9, interior 6..9 x 5..6, the four corners (3|12, 2|9) untouched
    "interior": ([[4, 3, 11, 8]], [1], None, [
        "................",
        "................",
        "....########....",
        "...##########...",
        "...##########...",
        "...###....###...",
        "...###....###...",
        "...##########...",
        "...##########...",
        "....########....",
        "................",
        "................"]),
    # (-3, -2)..(5, 4): outer -4..6 x -3..5 clipped at the left and the top border, interior -1..3 x 0..2, one corner (6, 5) in the image
    "clipped at two borders": ([[-3, -2, 5, 4]], [1], None, [
        "....###.........",
        "....###.........",
        "....###.........",
        "#######.........",
        "#######.........",
        "######..........",
        "................",
        "................",
        "................",
        "................",
        "................",
        "................"]),
    "entirely outside": ([[20, 3, 30, 8], [-10, -10, -3, -3], [2, 14, 9, 30], [3, -9, 8, -2]], [1, 2, 1, 2], None, ["................"] * 12),
    # a vertical line x = 5, y = 4..9 (outer 4..6 x 3..10 minus its corners) and a point (12, 6): a plus
    "degenerate": ([[5, 4, 5, 9], [12, 6, 12, 6]], [1, 1], None, [
        "................",
        "................",
        "................",
        ".....#..........",
        "....###.........",
        "....###.....#...",
        "....###....###..",
        "....###.....#...",
        "....###.........",
        "....###.........",
        ".....#..........",
        "................"]),
    # a = (2, 2)..(9, 8) drawn first, b = (6, 5)..(13, 10) second: b wins where both paint, a shows through b's interior (8..11 x 7..8)
    "later box wins": ([[2, 2, 9, 8], [6, 5, 13, 10]], [1, 2], None, [
        "................",
        "..aaaaaaaa......",
        ".aaaaaaaaaa.....",
        ".aaaaaaaaaa.....",
        ".aaa..bbbbbbbb..",
        ".aaa.bbbbbbbbbb.",
        ".aaa.bbbbbbbbbb.",
        ".aaaabbbaaa.bbb.",
        ".aaaabbbaaa.bbb.",
        "..aaabbbbbbbbbb.",
        ".....bbbbbbbbbb.",
        "......bbbbbbbb.."]),
    # score 0.5 is not above 0.5; float32(0.5000001) is
    "score threshold": ([[1, 1, 4, 4], [10, 6, 10, 6]], [1, 2], [0.5, 0.5000001], [
        "................",
        "................",
        "................",
        "................",
        "................",
        "..........b.....",
        ".........bbb....",
        "..........b.....",
        "................",
        "................",
        "................",
        "................"]),
    # (-0.9, -0.5, 5.99, 4.2) -> (0, 0, 5, 4), toward zero: interior 2..3 x 2..2 (floor would give -1, -1 and an interior 1..3 x 1..2)
    "truncation toward zero": ([[-0.9, -0.5, 5.99, 4.2]], [1], None, [
        "#######.........",
        "#######.........",
        "##..###.........",
        "#######.........",
        "#######.........",
        "######..........",
        "................",
        "................",
        "................",
        "................",
        "................",
        "................"]),
}
LEGEND = {"#": 1, "a": 1, "b": 2}


def case_inputs(name):
    boxes, labels, scores, picture = CASES[name]
    return (torch.tensor(boxes, dtype=torch.float32), torch.tensor(labels, dtype=torch.int64),
            None if scores is None else torch.tensor(scores, dtype=torch.float32), picture)


def test_label_colours_are_the_references():
    got = overlay.compute_colors_for_labels(torch.arange(91))
    assert got.shape == (91, 3) and got.dtype == np.float64 and np.array_equal(got, np.asarray(GOLDEN["colors"]))
    assert utils.compute_colors_for_labels is overlay.compute_colors_for_labels
    assert utils.create_unique_color_float(7) == tuple(c for c in utils.create_unique_color_float(7, hue_step=0.05))
    assert overlay.label_rgb(torch.arange(91)) == GOLDEN["rgb"]
    assert overlay.label_rgb([90, 1, 1]) == [GOLDEN["rgb"][90], GOLDEN["rgb"][1], GOLDEN["rgb"][1]]
    # the two things the reference does to a colour, both kept: red and blue swapped, cv2's rounding (label 1: (170, 114.75, 0))
    assert unpack(GOLDEN["rgb"][1]) == [0, 115, 170]
    assert len(set(GOLDEN["rgb"][1:])) > 40 and GOLDEN["rgb"][1] != GOLDEN["rgb"][2] != 0
    assert overlay.label_rgb([91])[0] == overlay._pack_rgb(overlay.compute_colors_for_labels([91])[0])      # outside the table: computed


@pytest.mark.parametrize("name", sorted(CASES))
def test_render_host_draws_the_rule(name):
    boxes, labels, scores, picture = case_inputs(name)
    image, _ = background()
    got = overlay.render_host(image, boxes, labels, scores)
    want = expected(picture, LEGEND)
    assert got.dtype == np.uint8 and got.shape == (H, W, 3) and got.flags["C_CONTIGUOUS"]
    assert np.array_equal(got, want), "\n".join("".join("#" if (got[y, x] != background()[1][y, x]).any() else "." for x in range(W)) for y in range(H))


def test_the_four_outer_corner_pixels_stay_untouched():
    image, plain = background()
    got = overlay.render_host(image, torch.tensor([[4., 3., 11., 8.]]), torch.tensor([1]))
    for y in (2, 9):
        for x in (3, 12):
            assert np.array_equal(got[y, x], plain[y, x])
            assert not np.array_equal(got[y, x + (1 if x == 3 else -1)], plain[y, x + (1 if x == 3 else -1)])


def test_overlay_boxes_torch_returns_the_references_bgr_array():
    boxes, labels, _, picture = case_inputs("later box wins")
    image, _ = background()
    got = utils.overlay_boxes_torch(image, {"boxes": boxes, "labels": labels})            # no scores: every box
    assert np.array_equal(got[:, :, ::-1], expected(picture, LEGEND)) and got.flags["C_CONTIGUOUS"]
    got = utils.overlay_boxes_torch(image.half(), {"boxes": boxes, "labels": labels, "scores": torch.tensor([0.9, 0.2])})
    assert np.array_equal(got[:, :, ::-1], overlay.render_host(image.half(), boxes[:1], labels[:1]))


def _rule(values):
    """k = trunc(float32(x) * 255.0f), saturated, NaN -> 0, from exact arithmetic: the float64 product of a float32 and 255 is exact,
    and rounding it to float32 once is the float32 multiplication"""
    prod = (values.astype(np.float64) * 255.0).astype(np.float32).astype(np.float64)
    return np.where(np.isnan(prod), 0, np.clip(np.trunc(np.nan_to_num(prod, nan=0.0)), 0, 255)).astype(np.uint8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_pixel_conversion(dtype):
    k = np.arange(256)
    values = np.concatenate([k / 255.0, (k + 0.999) / 255.0, [1.0, 1.0 + 2.0 ** -10]])
    t = torch.tensor(values, dtype=torch.float64).to(dtype)
    got = overlay.to_rgb8_host(t.reshape(1, 1, -1).expand(3, 1, -1))
    assert got.shape == (1, values.size, 3) and np.array_equal(got[0, :, 0], got[0, :, 2])
    got = got[0, :, 0]
    assert np.array_equal(got, _rule(t.double().numpy()))
    assert got[512] == 255 and got[513] == 255                                   # 1.0 and one Half ulp above it (saturated)
    if dtype == torch.float32:                                                   # ToTensor -> ToPILImage round trip, and truncation
        assert np.array_equal(got[:256], k) and np.array_equal(got[256:512], k)
    else:                                                                        # Half cannot hold k / 255: off by one below, never above
        assert np.all((got[:256] == k) | (got[:256] == k - 1)) and got[255] == 255 and got[0] == 0
    odd = torch.tensor([float("nan"), -0.25, -float("inf"), 2.0, float("inf"), 256 / 255.0, 1.01], dtype=dtype)
    assert overlay.to_rgb8_host(odd.reshape(1, 1, -1).expand(3, 1, -1))[0, :, 1].tolist() == [0, 0, 0, 255, 255, 255, 255]


# ---- engine.evaluate ------------------------------------------------------------------------------------------------------------------

class FixedDetector(torch.nn.Module):
    """stands in for the detector: image number i of the run gets DETECTIONS[i]"""

    def __init__(self, detections):
        super().__init__()
        self.detections, self.seen = detections, []

    def forward(self, images, **kw):
        self.seen.append(images[0].detach().clone())
        return [{k: v.clone() for k, v in self.detections[len(self.seen) - 1].items()}]


def fixed_detections(h, w):
    g = torch.Generator().manual_seed(5)
    out = []
    for n in (4, 0, 9):
        xy = torch.rand(n, 2, generator=g) * torch.tensor([w - 8.0, h - 8.0])
        out.append({"boxes": torch.cat([xy, xy + 2 + torch.rand(n, 2, generator=g) * torch.tensor([w / 2.0, h / 2.0])], dim=1),
                    "labels": torch.randint(1, 91, (n,), generator=g), "scores": torch.linspace(0.95, 0.3, n)})
    return out


def synthetic_loader(h, w, n=3, **tf):
    from detectinblur_amd.coco_utils import SyntheticCocoDetection
    from detectinblur_amd.train import get_transform
    with contextlib.redirect_stdout(io.StringIO()):
        ds = SyntheticCocoDetection(num_images=n, size=(h, w), boxes_per_image=2, transforms=get_transform(False, **tf))

    class L(list):
        dataset = ds
    return L(utils.collate_fn([ds[i]]) for i in range(n))


def read_png(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "RGB"
        return np.array(im)


def test_evaluate_writes_one_picture_per_image_cpu(tmp_path):
    """reference engine.py:382-383.  Fails on a tree where `image_output_folder` is accepted and dropped: no file appears."""
    from detectinblur_amd import engine
    h, w = 40, 56
    dets = fixed_detections(h, w)
    model = FixedDetector(dets)
    folder = tmp_path / "not" / "there" / "yet"                          # created (the reference crashes)
    with contextlib.redirect_stdout(io.StringIO()):
        out = engine.evaluate(model, synthetic_loader(h, w), torch.device("cpu"), vanilla_eval=True, image_output_folder=str(folder))
    assert sorted(os.listdir(folder)) == ["img0.png", "img1.png", "img2.png"]
    assert len(model.seen) == 3 and len(out["detections"]) == 3
    assert sum(int((d["scores"] > 0.5).sum()) for d in dets) > 5
    for i, (image, det) in enumerate(zip(model.seen, dets)):
        want = overlay.render_host(image, det["boxes"], det["labels"], det["scores"])
        assert want.shape == (h, w, 3) and np.array_equal(read_png(folder / ("img%d.png" % i)), want), i
    plain = overlay.render_host(model.seen[0], dets[0]["boxes"][:0], dets[0]["labels"][:0])
    assert not np.array_equal(read_png(folder / "img0.png"), plain) and np.array_equal(read_png(folder / "img1.png"),
                                                                                      overlay.to_rgb8_host(model.seen[1]))


def test_evaluate_without_a_folder_writes_nothing(tmp_path, monkeypatch):
    from detectinblur_amd import engine
    monkeypatch.chdir(tmp_path)
    model = FixedDetector(fixed_detections(40, 56))
    with contextlib.redirect_stdout(io.StringIO()):
        engine.evaluate(model, synthetic_loader(40, 56), torch.device("cpu"), vanilla_eval=True)
    assert os.listdir(tmp_path) == []


class _Stop(Exception):
    pass


@pytest.mark.parametrize("argv, want", [
    (["--vanilla_eval"], None), (["--vanilla_eval", "--save_images"], os.path.join("pics", "clean")),
    ([], None), (["--save_images"], os.path.join("pics", "P0.005_E0.04"))])
def test_driver_hands_a_folder_per_pass_only_with_save_images(monkeypatch, argv, want):
    from detectinblur_amd import evaluate as EV
    parser = EV.build_parser()
    assert "--save_images" in {s for a in parser._actions for s in a.option_strings}
    assert parser.parse_args([]).save_images is False and parser.parse_args([]).image_output_dir == "debug"
    seen = []

    def fake_evaluate(*a, **k):
        seen.append(k)
        raise _Stop()
    monkeypatch.setattr(EV, "evaluate", fake_evaluate)
    monkeypatch.setattr(EV, "fasterrcnn_resnet50_fpn", lambda **k: torch.nn.Linear(1, 1))
    args = parser.parse_args(["--synthetic", "--synthetic_images", "2", "--synthetic_size", "64", "64", "--device", "cpu", "-j", "0",
                              "--image_output_dir", "pics"] + argv)
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(_Stop):
        EV.main(args)
    assert len(seen) == 1 and "image_output_folder" in seen[0] and seen[0]["image_output_folder"] == want


def test_sweep_cells_get_fifteen_different_folders():
    from detectinblur_amd import evaluate as EV
    names = ["P%g_E%g" % (p, f) for p in EV.SWEEP_PARAMS for f in EV.SWEEP_FRACTIONS]
    assert len(set(names)) == 15 and names[0] == "P0.005_E0.04" and names[-1] == "P5e-05_E1"


# ---- the C entry point and the writer -----------------------------------------------------------------------------------------------

def test_overlay_argument_errors_are_reported_without_a_gpu():
    from detectinblur_amd import _lib
    l = _lib.lib()
    fake = _lib.ptr_array([4096])                                        # never dereferenced: every call below fails its checks first
    one, two = _lib.int_array([2]), _lib.int_array([0, 0])

    def call(in_dev=fake, dtype=_lib.DIB_F16, H=one, W=one, B=1, boxes=None, offset=two, out_dev=fake):
        return l.dib_overlay_rgb8(in_dev, dtype, H, W, B, boxes, offset, out_dev, None)
    for kw in (dict(in_dev=None), dict(H=None), dict(W=None), dict(offset=None), dict(out_dev=None), dict(in_dev=_lib.ptr_array([None])),
               dict(offset=_lib.int_array([0, 3]))):                     # boxes announced, none given
        assert call(**kw) == _lib.DIB_EINVAL and b"null pointer" in l.dib_last_error(), kw
    assert call(H=_lib.int_array([0])) == _lib.DIB_EINVAL and b"H, W > 0" in l.dib_last_error()
    assert call(W=_lib.int_array([-5])) == _lib.DIB_EINVAL and b"H, W > 0" in l.dib_last_error()
    assert call(offset=_lib.int_array([3, 1]), boxes=4096) == _lib.DIB_EINVAL and b"decreases" in l.dib_last_error()
    assert call(offset=_lib.int_array([-1, 1]), boxes=4096) == _lib.DIB_EINVAL and b"negative" in l.dib_last_error()
    assert call(dtype=7) == _lib.DIB_EINVAL and b"dtype" in l.dib_last_error()
    assert call(B=33) == _lib.DIB_EINVAL and b"32" in l.dib_last_error()
    assert call(H=_lib.int_array([1 << 16]), W=_lib.int_array([(1 << 14) + 1])) == _lib.DIB_EINVAL and b"2^30" in l.dib_last_error()
    assert call(B=0) == 0


def test_png_writer_reraises_a_workers_error_and_bounds_its_ring(tmp_path, monkeypatch):
    gate, calls = threading.Event(), []

    def save(path, rgb):
        gate.wait()
        calls.append(os.path.basename(path))
        if path.endswith("img1.png"):
            raise ValueError("disk full")
    monkeypatch.setattr(overlay, "save_png", save)
    w = overlay.PngWriter(tmp_path / "new", workers=1, depth=2)
    assert os.path.isdir(tmp_path / "new") and w.path(7) == str(tmp_path / "new" / "img7.png")
    w.submit(0, np.zeros((2, 2, 3), dtype=np.uint8))
    w.submit(1, torch.zeros((2, 2, 3), dtype=torch.uint8))
    assert not w._free.acquire(blocking=False)                           # both slots on their way: a third submit would wait here
    gate.set()
    with pytest.raises(ValueError, match="disk full"):
        w.close()
    assert calls == ["img0.png", "img1.png"]
    w.close()                                                            # idempotent
    with pytest.raises(RuntimeError):
        w.submit(2, np.zeros((2, 2, 3), dtype=np.uint8))


def test_png_writer_writes_what_it_is_given(tmp_path):
    rs = np.random.RandomState(0)
    pictures = [rs.randint(0, 256, (5 + i, 7, 3), dtype=np.uint8) for i in range(11)]
    w = overlay.PngWriter(tmp_path, workers=4, depth=3)
    for i, p in enumerate(pictures):
        w.submit(i, p)
    w.close()
    for i, p in enumerate(pictures):
        assert np.array_equal(read_png(tmp_path / ("img%d.png" % i)), p)
