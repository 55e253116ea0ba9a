"""The blur's whole dispatch matrix, once, at small shapes: accumulation mode x PSF canvas x launch path.

Every combination the library serves must give the bits of the generic kernel (dib_sparse_blur_generic: direct global reads, one
thread per pixel, no tiles, no LDS window) on the same tap table -- dtype 0 / 2 / 3 for bitexact / fp32 / fma16.  fast16 reorders
taps, so it has no second implementation: its served paths must agree bit for bit among themselves and stay within
blur_ops.ACC_MODE_TOLERANCE["fast16"] of the bit-exact result.  Every combination the library does not serve must be answered
the way it is today: DIB_EINVAL with its text, `None` / return value 1 from the fused normalising launch.

Paths: a uniform batch (2-D grid), a ragged batch (1-D flat grid), the same with dib_debug_set_flat_grid(0), the 256-wide tile
shape (dib_debug_set_shape(1)), the large window, sparse_blur_normalized (planar and channels-last), blur_step on the library's
buffers (single launch on and off, large window asked for) and dib_blur_step_packed on caller tables; plus fp32 images and a batch of
more than 32 images, which go through the same batch builder.

Shapes: 3 x 40 x 150 has a partial tile row and an edge tile of 22 valid columns; the ragged batch is 12 / 6 / 18 / 2 tiles with
zero padding (a side below 64) and reflect padding; no side is 64.  PSFs spread over more than 13 rows and 25 columns, so every
image takes several window refills; the large window's PSF is 16 rows x 48 columns."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MODES = ["bitexact", "fp32", "fma16", "fast16"]
GENERIC_DTYPE = {"bitexact": 0, "fp32": 2, "fma16": 3}
UNIFORM = [(3, 40, 150)] * 2
RAGGED = [(3, 40, 150), (1, 33, 300), (3, 70, 130), (2, 50, 60)]
NORM = [(3, 40, 150), (3, 33, 130)]      # into 64 x 256: the images' own tiles cover it
HP, WP = 64, 256


def _psf(rs, K, rows, cols, n, centre):
    """n random taps in a rows x cols box around `centre` of the K canvas (its corners set, so the extent is exact), fp16, sum ~1."""
    a = np.zeros((K, K), np.float64)
    r0, c0 = centre[0] - rows // 2, centre[1] - cols // 2
    a[r0 + rs.randint(0, rows, n), c0 + rs.randint(0, cols, n)] = rs.random_sample(n) + 0.05
    a[r0, c0] = a[r0 + rows - 1, c0 + cols - 1] = 0.5
    return torch.from_numpy((a / a.sum()).astype(np.float16)).cuda()


def _images(rs, shapes, dtype=np.float16):
    return [torch.from_numpy(rs.random_sample(s).astype(dtype)).cuda() for s in shapes]


class World(object):
    """Inputs, tap tables and the generic kernel's results, made once for the module and left unchanged."""

    def __init__(self):
        from detectinblur_amd import _lib, blur_ops
        self.L, self.ops, self.lib = _lib, blur_ops, _lib.lib()
        for hook in (self.lib.dib_debug_set_shape, self.lib.dib_debug_set_flat_grid, self.lib.dib_debug_set_step_fused):
            hook.argtypes, hook.restype = [ctypes.c_int], None
        rs = np.random.RandomState(20260)
        self.images = {"uniform": _images(rs, UNIFORM), "ragged": _images(rs, RAGGED), "norm": _images(rs, NORM)}
        self.images["uniform"][0] = self.images["ragged"][0]          # one image and PSF in both batches: fast16 must agree across them
        self.means, self.stds = rs.uniform(0.2, 0.6, (2, 3)), rs.uniform(0.15, 0.35, (2, 3))
        self.psfs, self.tables, self._ref = {}, {}, {}
        for K in (128, 256):
            centre = (63, 63) if K == 128 else (147, 112)             # off-centre on the 256 canvas
            self.psfs[K] = [_psf(rs, K, 21, 41, 40, centre) for _ in RAGGED]
            self.psfs[K, "large"] = [_psf(rs, K, 16, 48, 60, centre) for _ in RAGGED]
            self.tables[K, "std"] = blur_ops.compact_psfs(self.psfs[K], True)
            self.tables[K, "vruns"] = blur_ops.compact_psfs(self.psfs[K], True, vruns=True)
            self.tables[K, "large"] = blur_ops.compact_psfs(self.psfs[K, "large"], True, large_window=True)
        torch.cuda.synchronize()

    def stream(self):
        return torch.cuda.current_stream().cuda_stream

    def generic(self, batch, K, mode, which="std"):
        """The generic kernel's result for every image of `batch` with PSF i for image i (cached)."""
        key = (batch, K, mode, which)
        if key not in self._ref:
            outs, tabs = [], self.tables[K, which]
            for i, img in enumerate(self.images[batch]):
                out = torch.empty_like(img)
                C, H, W = img.shape
                self.L.check(self.lib.dib_sparse_blur_generic(img.data_ptr(), out.data_ptr(), C, H, W, GENERIC_DTYPE[mode], tabs.ptr(i), K, self.stream()))
                outs.append(out)
            self._ref[key] = outs
        return self._ref[key]

    def sparse_blur(self, images, tabs, K, acc_word, index=None, dtype=0):
        """dib_sparse_blur itself: (return code, outputs)."""
        outs = [torch.empty_like(t) for t in images]
        arr = self.L.int_array
        rc = self.lib.dib_sparse_blur(self.L.ptr_array([t.data_ptr() for t in images]), self.L.ptr_array([t.data_ptr() for t in outs]),
                                      arr([t.shape[0] for t in images]), arr([t.shape[1] for t in images]), arr([t.shape[2] for t in images]),
                                      arr(index if index is not None else list(range(len(images)))), len(images), dtype, tabs.buf.data_ptr(),
                                      tabs.count, K, acc_word, self.stream())
        return rc, outs

    def step_packed(self, images, psfs, K, acc, tabs, flags=0):
        """dib_blur_step_packed on caller tables: (return code, outputs)."""
        outs = [torch.empty_like(t) for t in images]
        n = len(images)
        ptrs = self.L.ptr_array([p.data_ptr() for p in psfs] + [t.data_ptr() for t in images] + [t.data_ptr() for t in outs])
        ints = self.L.int_array([t.shape[0] for t in images] + [t.shape[1] for t in images] + [t.shape[2] for t in images] + list(range(n)))
        rc = self.lib.dib_blur_step_packed(ptrs, ints, 0, len(psfs), K, 1, n, 0, acc, tabs.buf.data_ptr(), flags, self.stream())
        return rc, outs

    def normalized(self, K, acc, tabs, channels_last):
        """dib_sparse_blur_normalized itself on the `norm` images: (return code, output batch)."""
        imgs = self.images["norm"]
        fmt = torch.channels_last if channels_last else torch.contiguous_format
        out = torch.full((2, 3, HP, WP), 7.0, dtype=torch.float32, device="cuda").contiguous(memory_format=fmt)
        m, sd = (np.ascontiguousarray(a, dtype=np.float32) for a in (self.means, self.stds))
        fp = ctypes.POINTER(ctypes.c_float)
        arr = self.L.int_array
        rc = self.lib.dib_sparse_blur_normalized(self.L.ptr_array([t.data_ptr() for t in imgs]), arr([t.shape[1] for t in imgs]), arr([t.shape[2] for t in imgs]),
                                                 arr([0, 1]), arr([0, 1]), 2, tabs.buf.data_ptr(), tabs.count, K, acc, m.ctypes.data_as(fp),
                                                 sd.ctypes.data_as(fp), out.data_ptr(), HP, WP, int(channels_last), self.stream())
        return rc, out

    def error(self):
        return self.lib.dib_last_error().decode()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.lib.dib_debug_set_shape(0); w.lib.dib_debug_set_flat_grid(1); w.lib.dib_debug_set_step_fused(1)


def _same(got, want):
    assert len(got) == len(want)
    for g, x in zip(got, want):
        assert g.shape == x.shape and torch.equal(g.view(torch.int16), x.view(torch.int16))


_fast16 = {}      # (batch, image) -> the first served path's fast16 result: every later path must give the same bits


def _check_served(w, batch, K, mode, outs, which="std", ref_mode=None):
    if (ref_mode or mode) != "fast16":
        return _same(outs, w.generic(batch, K, ref_mode or mode, which))
    exact = w.generic(batch, K, "bitexact")
    for i, (o, e) in enumerate(zip(outs, exact)):
        key = (batch, i) if not (batch == "uniform" and i == 0) else ("ragged", 0)
        first = _fast16.setdefault(key, o)
        assert torch.equal(o.view(torch.int16), first.view(torch.int16)), "fast16 differs between two paths (image %d)" % i
        worst = float((o.float() - e.float()).abs().max())
        print("fast16 vs bitexact, %s image %d: max abs %.3g" % (batch, i, worst))
        assert worst <= w.ops.ACC_MODE_TOLERANCE["fast16"]


DIRECT = {"uniform": ("uniform", 1, 0), "ragged_flat": ("ragged", 1, 0), "ragged_2d": ("ragged", 0, 0), "shape_256": ("ragged", 1, 1)}


@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", list(DIRECT))
def test_sparse_blur(world, path, mode, K):
    w = world
    batch, flat, shape = DIRECT[path]
    acc = w.ops.ACC_MODES[mode]
    w.lib.dib_debug_set_flat_grid(flat); w.lib.dib_debug_set_shape(shape)
    try:
        rc, outs = w.sparse_blur(w.images[batch], w.tables[K, "vruns" if mode == "fast16" else "std"], K, acc)
    finally:
        w.lib.dib_debug_set_flat_grid(1); w.lib.dib_debug_set_shape(0)
    if mode == "fast16" and (K != 128 or shape):
        assert rc == w.L.DIB_EINVAL and "DIB_ACC_FAST16 serves K = 128 on the default tiles and the standard window" in w.error()
        with pytest.raises(w.ops.AccModeError):
            w.ops.resolve_acc_mode(mode, 256, torch.float16, substitute=False)
        return
    w.L.check(rc)
    _check_served(w, batch, K, mode, outs)


@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("mode", MODES)
def test_large_window(world, mode, K):
    w = world
    rc, outs = w.sparse_blur(w.images["ragged"][:2], w.tables[K, "large"], K, w.ops.ACC_MODES[mode] | w.L.DIB_WINDOW_LARGE)
    if mode == "fp32":
        assert rc == w.L.DIB_EINVAL and "DIB_WINDOW_LARGE serves fp16 images in DIB_ACC_BITEXACT / DIB_ACC_FMA16" in w.error()
    elif mode == "fast16":
        assert rc == w.L.DIB_EINVAL and "DIB_ACC_FAST16 serves K = 128 on the default tiles and the standard window" in w.error()
    else:
        w.L.check(rc)
        _same(outs, w.generic("ragged", K, mode, "large")[:2])
    if mode in ("fp32", "fast16"):      # the one place that decides (resolve_acc_mode) keeps those modes off the large window
        assert w.ops.resolve_acc_mode(mode, 128, torch.float16, large_window=True)[2] is False


@pytest.mark.parametrize("channels_last", [False, True])
@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("mode", MODES)
def test_normalized(world, mode, K, channels_last):
    w = world
    acc = w.ops.ACC_MODES[mode]
    tabs = w.tables[K, "vruns" if mode == "fast16" else "std"]
    rc, out = w.normalized(K, acc, tabs, channels_last)
    if mode == "fast16" and K != 128:
        assert rc == 1 and bool((out == 7.0).all())            # not served, nothing launched
        assert w.ops.sparse_blur_normalized(w.images["norm"], [0, 1], tabs, w.means, w.stds, HP, WP, channels_last, acc) is None
        return
    w.L.check(rc)
    if mode == "fast16":      # against the unfused fast16 launch on the same images, itself held to the bit-exact result
        rc, blurred = w.sparse_blur(w.images["norm"], tabs, K, acc)
        w.L.check(rc)
        _check_served(w, "norm", K, mode, blurred)
    else:
        blurred = w.generic("norm", K, mode)
    want = w.ops.normalize_pad(blurred, w.means, w.stds, HP, WP, channels_last)
    assert out.stride() == want.stride() and torch.equal(out, want)      # every pixel and every padding zero
    assert w.ops.sparse_blur_normalized(w.images["norm"], [0, -1], tabs, w.means, w.stds, HP, WP, channels_last, acc) is None


@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", ["single_launch", "two_launches", "large_window"])
def test_blur_step_library_buffers(world, path, mode, K):
    w = world
    large = path == "large_window"
    w.lib.dib_debug_set_step_fused(0 if path == "two_launches" else 1)
    try:
        images = w.images["ragged"][:2] if large else w.images["ragged"]
        psfs = w.psfs[K, "large"][:2] if large else w.psfs[K]
        outs = w.ops.blur_step(images, list(range(len(images))), psfs, True, w.ops.ACC_MODES[mode], large_window=large)
    finally:
        w.lib.dib_debug_set_step_fused(1)
    ran = "fma16" if mode == "fast16" and K != 128 else mode      # resolve_acc_mode: fast16 on the 256 canvas runs fma16's loop
    if large:
        ref = w.generic("ragged", K, "bitexact" if ran == "fast16" else ran, "large")[:2]
        if ran != "fast16":
            return _same(outs, ref)
        worst = max(float((o.float() - e.float()).abs().max()) for o, e in zip(outs, ref))
        print("fast16 vs bitexact, wide PSF: max abs %.3g" % worst)
        assert worst <= w.ops.ACC_MODE_TOLERANCE["fast16"]
        return
    _check_served(w, "ragged", K, mode, outs, ref_mode=ran)


@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("mode", MODES)
def test_blur_step_caller_tables(world, mode, K):
    w = world
    tabs = w.ops.TapTables(K, len(RAGGED), torch.device("cuda"))
    rc, outs = w.step_packed(w.images["ragged"], w.psfs[K], K, w.ops.ACC_MODES[mode], tabs)
    if mode == "fast16" and K != 128:      # the library itself substitutes nothing
        assert rc == w.L.DIB_EINVAL and "DIB_ACC_FAST16 serves K = 128" in w.error()
        return
    w.L.check(rc)
    _check_served(w, "ragged", K, mode, outs)


def test_fp32_images_and_a_batch_of_more_than_32(world):
    """fp32 images run the generic kernel behind dib_sparse_blur; 37 images (three of them skipped) take two launches."""
    w = world
    rs = np.random.RandomState(5)

    def generic(imgs, tabs, table, dtype):
        outs = [torch.empty_like(t) for t in imgs]
        for t, o, k in zip(imgs, outs, table):
            w.L.check(w.lib.dib_sparse_blur_generic(t.data_ptr(), o.data_ptr(), t.shape[0], t.shape[1], t.shape[2], dtype, tabs.ptr(k), 128, w.stream()))
        return outs

    tabs = w.ops.compact_psfs([p.float() for p in w.psfs[128]], True)      # fp32 images take fp32 weights
    imgs32 = _images(rs, RAGGED, np.float32)
    rc, outs = w.sparse_blur(imgs32, tabs, 128, 0, dtype=1)
    w.L.check(rc)
    for g, x in zip(outs, generic(imgs32, tabs, range(4), 1)):
        assert torch.equal(g.view(torch.int32), x.view(torch.int32)) and float(g.abs().max()) > 0.1
    tabs = w.tables[128, "std"]
    many = _images(rs, [(1, 20 + i % 3, 30 + i) for i in range(37)])
    index = [-1 if i in (0, 17, 36) else i % 4 for i in range(37)]
    rc, outs = w.sparse_blur(many, tabs, 128, 0, index)
    w.L.check(rc)
    live = [i for i in range(37) if index[i] >= 0]
    _same([outs[i] for i in live], generic([many[i] for i in live], tabs, [index[i] for i in live], 0))
