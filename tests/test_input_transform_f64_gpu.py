"""The input transform kernels (csrc/dib_epilogue.hip: normalize_pad_kernel, normalize_resize_pad_kernel behind dib_normalize_pad,
dib_normalize_resize_pad and dib_normalize_resize_crop) against the host reference of oracle/dib_oracle.py A23, which no GPU kernel
has a part in: float16 and float32 images, planar and channels-last, contracted and uncontracted, on the small inputs of
tests/test_input_transform_reference.py -- NaN, +-inf, 65504, denormals and -0 among them.  One comparison function
(O.input_transform_compare): the non-finite classes by position, unit-scale and padding elements bit for bit, interpolated elements
within 5 * 2^-24 * M of the float64 value.  Also what a checker on the same GPU cannot see: the second launch chunk of all three
entry points, DIB_EPILOGUE_PAD alone, the sampling positions against real arithmetic (a ramp), images at odd element offsets, and
that every element of the batch is written and nothing behind it."""
import ctypes

import numpy as np
import pytest
import torch

import dib_oracle as O
from detectinblur_amd import _lib, blur_ops
from tests import test_input_transform_reference as R

pytestmark = pytest.mark.gpu
DTYPES = {"float16": np.float16, "float32": np.float32}
VARIANTS = {"contracted": 1, "uncontracted": 0}
DIB_F16, DIB_F32 = blur_ops._DT[torch.float16], blur_ops._DT[torch.float32]
SENTINEL, TAIL = -777.0, 64


class contraction:
    """dib_debug_set_resize_contraction for a block; the switch is process-wide, so the default comes back whatever happens"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.set(self.on)

    def __exit__(self, *exc):
        self.set(1)

    @staticmethod
    def set(on):
        fn = _lib.lib().dib_debug_set_resize_contraction
        fn.argtypes, fn.restype = [ctypes.c_int], None
        fn(int(on))


def _device(images):
    return [torch.from_numpy(i).cuda() for i in images]


def wrapper(case, channels_last, images=None):
    """through blur_ops: normalize_crop for a crop, normalize_pad otherwise (dib_normalize_pad when no image is resized)"""
    images = _device(case["images"]) if images is None else images
    fn = blur_ops.normalize_crop if case["crop"] else blur_ops.normalize_pad
    out = fn(images, case["means"], case["stds"], case["Hp"], case["Wp"], channels_last, out_sizes=case["out_sizes"], quantize=case["quantize"])
    assert out.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
    return out.cpu().numpy()


def abi(entry, case, channels_last, flags=0):
    """One entry point straight through the C ABI into a buffer pre-filled with a sentinel, TAIL floats longer than the batch:
    every element of the batch is overwritten, the tail is untouched.  Returns the batch [B, 3, Hp, Wp] (numpy)."""
    images = _device(case["images"])
    B, Hp, Wp = len(images), case["Hp"], case["Wp"]
    count = B * 3 * Hp * Wp
    buf = torch.full((count + TAIL,), SENTINEL, dtype=torch.float32, device="cuda")
    fp = ctypes.POINTER(ctypes.c_float)
    m = np.ascontiguousarray(np.asarray(case["means"], dtype=np.float64).reshape(B, 3).astype(np.float32))
    sd = np.ascontiguousarray(np.asarray(case["stds"], dtype=np.float64).reshape(B, 3).astype(np.float32))
    head = (_lib.ptr_array([i.data_ptr() for i in images]), DIB_F16 if images[0].dtype == torch.float16 else DIB_F32,
            _lib.int_array([i.shape[1] for i in images]), _lib.int_array([i.shape[2] for i in images]))
    sizes = (_lib.int_array([o[0] for o in case["out_sizes"]]), _lib.int_array([o[1] for o in case["out_sizes"]]))
    tail = (B, m.ctypes.data_as(fp), sd.ctypes.data_as(fp), buf.data_ptr(), Hp, Wp, int(channels_last))
    stream = _lib.stream_of(buf)
    l = _lib.lib()
    if entry == "dib_normalize_pad":
        assert all(tuple(o) == tuple(i.shape[1:]) for o, i in zip(case["out_sizes"], images)) and not case["quantize"]
        _lib.check(l.dib_normalize_pad(*head, *tail, stream))
    elif entry == "dib_normalize_resize_pad":
        _lib.check(l.dib_normalize_resize_pad(*head, *sizes, *tail, stream))
    else:
        _lib.check(l.dib_normalize_resize_crop(*head, *sizes, *tail, flags, stream))
    got = buf.cpu().numpy()
    assert (got[count:].view(np.uint32) == np.float32(SENTINEL).view(np.uint32)).all(), "%s wrote behind the batch" % entry
    left = int((got[:count].view(np.uint32) == np.float32(SENTINEL).view(np.uint32)).sum())
    assert left == 0, "%s left %d of %d elements unwritten" % (entry, left, count)
    got = got[:count]
    return got.reshape(B, Hp, Wp, 3).transpose(0, 3, 1, 2) if channels_last else got.reshape(B, 3, Hp, Wp)


def entries_of(case):
    """(entry point, flags) that take the case as it is"""
    if case["crop"]:
        return [("dib_normalize_resize_crop", _lib.DIB_EPILOGUE_QUANTIZE if case["quantize"] else 0)]
    if case["quantize"]:
        return [("dib_normalize_resize_crop", _lib.DIB_EPILOGUE_QUANTIZE | _lib.DIB_EPILOGUE_PAD)]
    unit = all(tuple(o) == i.shape[1:] for o, i in zip(case["out_sizes"], case["images"]))
    return ([("dib_normalize_pad", 0)] if unit else []) + [("dib_normalize_resize_pad", 0), ("dib_normalize_resize_crop", _lib.DIB_EPILOGUE_PAD)]


def check(case, channels_last, tag):
    """wrapper and every ABI entry point that takes the case, contracted and uncontracted, against the reference"""
    peaks = {}
    for variant, on in VARIANTS.items():
        ref = R.reference(case, contracted=bool(on))
        with contraction(on):
            runs = [("blur_ops", wrapper(case, channels_last))] + [(e, abi(e, case, channels_last, f)) for e, f in entries_of(case)]
        for name, got in runs:
            try:
                units = O.input_transform_compare(got, *ref)
            except AssertionError as e:
                raise AssertionError("%s, %s, %s: %s" % (tag, variant, name, e)) from None
            peaks[variant] = max(peaks.get(variant, 0.0), units)
    print("GPU %-28s %s" % (tag, ", ".join("%s peak %.2f x 2^-24 M" % kv for kv in peaks.items())))
    assert all(p <= O.TRANSFORM_BOUND for p in peaks.values())
    return peaks


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("layout", list(R.LAYOUTS))
def test_kernels_against_the_host_reference(layout, dtype, channels_last):
    peaks = check(R.build(R.LAYOUTS[layout], DTYPES[dtype], 1 + len(layout)), channels_last, "%s/%s/%s" % (layout, dtype, "nhwc" if channels_last else "nchw"))
    assert (layout == "unit") == (max(peaks.values()) == 0.0)                    # an interpolating case does round


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("kind", list(R.BATCH33))
def test_33_images_cross_the_launch_chunk_in_every_entry_point(kind, dtype, channels_last):
    """unit: dib_normalize_pad, dib_normalize_resize_pad, dib_normalize_resize_crop with DIB_EPILOGUE_PAD; resize: the latter two;
    crop: dib_normalize_resize_crop.  Every image has its own statistics: image 32 with image 0's would be a wrong value."""
    case = R.build33(kind, DTYPES[dtype])
    v = R.reference(case)[0]
    assert not np.array_equal(v[32], v[0]) and np.abs(v[32] - v[0]).max() > 1e-3
    check(case, channels_last, "batch33/%s/%s" % (kind, dtype))


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("kind", list(R.QUANT))
def test_quantised_source_pixels_in_pad_and_crop_mode(kind, channels_last):
    check(R.build_quant(kind), channels_last, "quantise/%s" % kind)


def same_bits(a, b):
    """bit for bit, NaN payloads included: both sides are the same kernel's stores"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_the_pad_flag_alone_equals_dib_normalize_resize_pad_bit_for_bit(dtype):
    case = R.build(R.RESIZE_PAD, DTYPES[dtype], 21)
    for channels_last in (False, True):
        a = abi("dib_normalize_resize_crop", case, channels_last, _lib.DIB_EPILOGUE_PAD)
        b = abi("dib_normalize_resize_pad", case, channels_last)
        assert same_bits(a, b)
    with pytest.raises(_lib.DibError, match="unknown flags"):
        abi("dib_normalize_resize_crop", case, False, 4)


RAMPS = [((37, 53), (64, 91)), ((70, 100), (33, 47)), ((9, 260), (9, 300)), ((40, 30), (13, 90)), ((3, 1), (96, 32)), ((128, 200), (32, 48))]


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_sampling_positions_on_a_ramp_against_real_arithmetic(dtype):
    """p[y][x] = (x + 3 y) / 2048 (exact in Half), mean 0, std 1: the output is (sx + 3 sy) / 2048 at the real-arithmetic positions
    s.  Tolerance (dw + 3 dh) / 2048 + 5 * 2^-24 * M with d = 3 * 2^-24 * (s + 1): one rounding of the scale, one of the product
    (uncontracted form) and one of the position itself, each at most 2^-24 of a magnitude <= s + 1."""
    sizes = RAMPS
    case = dict(images=[R.ramp_image(H, W, DTYPES[dtype]) for (H, W), _ in sizes], means=np.zeros((len(sizes), 3)), stds=np.ones((len(sizes), 3)),
                out_sizes=[o for _, o in sizes], Hp=96, Wp=320, crop=False, quantize=False)
    for variant, on in VARIANTS.items():
        M = R.reference(case, contracted=bool(on))[1]
        with contraction(on):
            got = wrapper(case, True).astype(np.float64)
        worst = 0.0
        for k, ((H, W), (Ho, Wo)) in enumerate(sizes):
            sy, sx = O.transform_positions(H, Ho)[4].reshape(-1, 1), O.transform_positions(W, Wo)[4].reshape(1, -1)
            want = (sx + 3.0 * sy) / 2048.0
            tol = (3 * 2.0 ** -24 * (sx + 1) + 3 * 3 * 2.0 ** -24 * (sy + 1)) / 2048.0 + O.TRANSFORM_BOUND * 2.0 ** -24 * M[k, :, :Ho, :Wo]
            err = np.abs(got[k, :, :Ho, :Wo] - want)
            assert (err <= tol).all(), (variant, (H, W), (Ho, Wo), float((err / tol).max()))
            worst = max(worst, float((err / tol).max()))
            assert not got[k, :, Ho:, :].any() and not got[k, :, :, Wo:].any()
        print("GPU ramp/%s %s: peak %.3f of the tolerance" % (dtype, variant, worst))


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_images_one_element_into_their_buffers_give_the_bits_of_aligned_copies(dtype):
    """float16 at an odd element offset (2-byte, not 4-byte aligned), float32 at 4-byte but not 16-byte alignment"""
    for layout in (R.UNIT, R.RESIZE_PAD, R.CROP_32):
        case = R.build(layout, DTYPES[dtype], 31)
        aligned = _device(case["images"])
        shifted = []
        for img in aligned:
            buf = torch.empty(img.numel() + 1, dtype=img.dtype, device="cuda")
            view = buf[1:].view(img.shape)
            view.copy_(img)
            assert view.is_contiguous() and view.data_ptr() % 16 == img.element_size() and img.data_ptr() % 16 == 0
            shifted.append(view)
        for channels_last in (False, True):
            assert same_bits(wrapper(case, channels_last, shifted), wrapper(case, channels_last, aligned))
