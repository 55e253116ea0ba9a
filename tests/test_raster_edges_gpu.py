"""The PSF rasteriser (csrc/dib_raster.hip) at batch seams, small canvases and borders: every case of tests/_raster_cases.py against
dib_oracle's restatement of the reference, bit for bit (tests/test_raster_reference.py checks on the CPU that the cases have the
properties their names claim).  No comparison here has a tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import dib_oracle as O
from tests import _raster_cases as RC

pytestmark = pytest.mark.gpu

IN_CANVAS = RC.in_canvas_cases()
HIGH = RC.high_border_cases()
BATCHES = RC.batch_cases()
SENTINEL = 0xA5
BAND = 4096          # bytes on each side of a guarded buffer


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 2: np.uint16}[a.dtype.itemsize])


def _check(got64, got16, want, what):
    """got64 / got16: device results of one PSF; want: its float64 oracle PSF."""
    assert np.array_equal(_bits(got64.cpu().numpy()), _bits(want)), what + ": float64"
    assert np.array_equal(_bits(got16.cpu().numpy()), _bits(O.to_half_like_torch(want))), what + ": float16"


@pytest.mark.parametrize("center", [False, True], ids=["raw", "centred"])
@pytest.mark.parametrize("canvas", RC.CANVASES)
def test_every_in_canvas_case_matches_the_oracle(canvas, center):
    from detectinblur_amd import blur_ops
    cases = [c for c in IN_CANVAS if c[1] == canvas]
    assert len(cases) == {64: 30, 128: 24, 256: 18}[canvas]
    for case in cases:
        name, _, re, im, frac = case
        want = RC.expected(case)[1 if center else 0]
        traj = (re + 1j * im)[None]
        p64, p16 = blur_ops.rasterize_psfs(traj, [frac], canvas=canvas, center=center, out_n=canvas)
        assert p64.shape == p16.shape == (1, canvas, canvas)
        _check(p64[0], p16[0], want, name)
        if canvas == 256:
            c64, c16 = blur_ops.rasterize_psfs(traj, [frac], canvas=256, center=center, out_n=128)
            assert c64.shape == c16.shape == (1, 128, 128)
            _check(c64[0], c16[0], want[64:192, 64:192], name + " [64:192]")


def test_default_out_n_is_the_crop_only_when_centring_a_256_canvas():
    from detectinblur_amd import blur_ops
    for case in IN_CANVAS:
        name, canvas, re, im, frac = case
        if not name.startswith("truncation_"):
            continue
        raw, cen = RC.expected(case)
        traj = (re + 1j * im)[None]
        _check(*[p[0] for p in blur_ops.rasterize_psfs(traj, [frac], canvas=canvas, center=False)], raw, name)
        _check(*[p[0] for p in blur_ops.rasterize_psfs(traj, [frac], canvas=canvas, center=True)],
               cen[64:192, 64:192] if canvas == 256 else cen, name)


@pytest.mark.parametrize("case", BATCHES, ids=[c[0] for c in BATCHES])
def test_batches_over_several_launch_chunks(case):
    """One call per batch; every PSF against its own oracle result (its own trajectory and its own fraction), raw and centred; a second
    call on the same inputs gives the same bytes."""
    from detectinblur_amd import blur_ops
    name, canvas, traj, fracs = case
    raw, cen = RC.expected_batch(case)
    dev = torch.from_numpy(traj).cuda()
    r64, r16 = blur_ops.rasterize_psfs(dev, fracs, canvas=canvas, center=False)
    c64, c16 = blur_ops.rasterize_psfs(traj, fracs, canvas=canvas, center=True, out_n=canvas)
    again64, again16 = blur_ops.rasterize_psfs(dev, fracs, canvas=canvas, center=True, out_n=canvas)
    r64, r16, c64, c16 = r64.cpu().numpy(), r16.cpu().numpy(), c64.cpu().numpy(), c16.cpu().numpy()
    for b in range(len(fracs)):
        assert np.array_equal(_bits(r64[b]), _bits(raw[b])), "%s: raw PSF %d" % (name, b)
        assert np.array_equal(_bits(c64[b]), _bits(cen[b])), "%s: centred PSF %d" % (name, b)
    assert np.array_equal(_bits(r16), _bits(O.to_half_like_torch(raw)))
    assert np.array_equal(_bits(c16), _bits(O.to_half_like_torch(cen)))
    assert np.array_equal(_bits(again64.cpu().numpy()), _bits(c64)) and np.array_equal(_bits(again16.cpu().numpy()), _bits(c16))


@pytest.mark.parametrize("canvas", RC.CANVASES)
def test_high_border_on_the_device_drops_what_falls_outside(canvas):
    """include/dib.h, "Canvas border": a device-resident trajectory with floor(coord) >= canvas - 1 contributes the cells inside the
    canvas only, where the reference raises IndexError -- the reference's loop on a padded accumulator, cropped."""
    from detectinblur_amd import blur_ops
    cases = [c for c in HIGH if c[1] == canvas]
    assert len(cases) == 10
    for name, _, re, im, frac in cases:
        want = RC.psf_rasterize_dropping(re, im, frac, canvas)
        kind = name.split("_")[2]
        if name.endswith("_full") and kind in ("x", "xy"):
            assert want[:, canvas - 1].any(), name               # the sample's own column canvas - 1 is kept
        if name.endswith("_full") and kind in ("y", "xy"):
            assert want[canvas - 1, :].any(), name
        if name.endswith("_unexposed") or kind in ("far", "edge"):
            # "edge" sits on cell (canvas - 1, canvas - 1) itself, which is inside and is kept
            assert want[canvas - 1, canvas - 1] == (1 / 8 if (kind == "edge" and name.endswith("_full")) else 0), name
        dev = torch.from_numpy((re + 1j * im)[None]).cuda()
        p64, p16 = blur_ops.rasterize_psfs(dev, [frac], canvas=canvas, center=False)
        _check(p64[0], p16[0], want, name)
        assert np.array_equal(_bits(p64[0, canvas - 1].cpu().numpy()), _bits(want[canvas - 1])), name
        assert np.array_equal(_bits(p64[0, :, canvas - 1].cpu().numpy()), _bits(want[:, canvas - 1])), name
        c64, c16 = blur_ops.rasterize_psfs(dev, [frac], canvas=canvas, center=True, out_n=canvas)
        _check(c64[0], c16[0], O.psf_center(want), name + " centred")


def _guarded(nbytes):
    buf = torch.full((nbytes + 2 * BAND,), SENTINEL, dtype=torch.uint8, device="cuda")
    return buf, buf.data_ptr() + BAND


def _bands_intact(buf):
    h = buf.cpu().numpy()
    return bool((h[:BAND] == SENTINEL).all() and (h[-BAND:] == SENTINEL).all())


def test_only_the_stated_extents_are_written():
    """B = 65 (two launch chunks) at canvas 64 through the C entry point: psf64, psf16 and the workspace sit between sentinel bands."""
    from detectinblur_amd import _lib, blur_ops
    case = BATCHES[1]
    name, canvas, traj, fracs = case
    B, iters = traj.shape
    assert (canvas, B) == (64, 65)
    l = _lib.lib()
    n = canvas * canvas
    ws_bytes = l.dib_psf_rasterize_workspace_bytes(B, iters, canvas)
    assert ws_bytes == B * n * (8 + 16)
    b64, p64 = _guarded(B * n * 8)
    b16, p16 = _guarded(B * n * 2)
    bws, pws = _guarded(ws_bytes)
    dev = torch.view_as_real(torch.from_numpy(traj).cuda()).contiguous()
    _lib.check(l.dib_psf_rasterize(dev.data_ptr(), B, iters, (ctypes.c_double * B)(*fracs), canvas, 1, canvas, p64, p16, pws,
                                   blur_ops._stream()))
    torch.cuda.synchronize()
    assert _bands_intact(b64) and _bands_intact(b16) and _bands_intact(bws)
    cen = RC.expected_batch(case)[1]
    got64 = b64[BAND:-BAND].cpu().numpy().view(np.float64).reshape(B, canvas, canvas)
    got16 = b16[BAND:-BAND].cpu().numpy().view(np.float16).reshape(B, canvas, canvas)
    assert np.array_equal(_bits(got64), _bits(cen))
    assert np.array_equal(_bits(got16), _bits(O.to_half_like_torch(cen)))
    # the raw canvases are the first B * canvas^2 doubles of the workspace (include/dib.h does not promise it; the kernel does)
    raw = bws[BAND:BAND + B * n * 8].cpu().numpy().view(np.float64).reshape(B, canvas, canvas)
    assert np.array_equal(_bits(raw), _bits(RC.expected_batch(case)[0]))


def test_refusals_and_the_empty_batch():
    """Every refused call is made with real device buffers sized for one canvas-256 PSF, so that a missing refusal stays inside an
    allocation; nothing is written by a refused call or by B == 0."""
    from detectinblur_amd import _lib, blur_ops
    l = _lib.lib()
    iters, n = 300, 256 * 256
    traj = torch.full((1, iters, 2), 128.25, dtype=torch.float64, device="cuda")
    out64 = torch.full((n * 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    out16 = torch.full((n * 2,), SENTINEL, dtype=torch.uint8, device="cuda")
    ws = torch.full((l.dib_psf_rasterize_workspace_bytes(1, iters, 256),), SENTINEL, dtype=torch.uint8, device="cuda")
    fr = (ctypes.c_double * 1)(0.5)
    T, W, S = traj.data_ptr(), ws.data_ptr(), blur_ops._stream()

    def call(traj=T, B=1, iters=iters, fraction=fr, canvas=256, center=1, out_n=256, workspace=W):
        code = l.dib_psf_rasterize(traj, B, iters, fraction, canvas, center, out_n, out64.data_ptr(), out16.data_ptr(), workspace, S)
        return code, l.dib_last_error().decode()

    refused = [
        (dict(canvas=32, out_n=32), "canvas must be 64, 128 or 256, got 32"),
        (dict(canvas=100, out_n=100), "canvas must be 64, 128 or 256, got 100"),
        (dict(canvas=0, out_n=0), "canvas must be 64, 128 or 256, got 0"),
        (dict(canvas=128, out_n=64), "out_n must be canvas, or 128 with canvas 256"),
        (dict(canvas=128, out_n=256), "out_n must be canvas, or 128 with canvas 256"),
        (dict(canvas=64, out_n=128), "out_n must be canvas, or 128 with canvas 256"),
        (dict(canvas=256, out_n=64), "out_n must be canvas, or 128 with canvas 256"),
        (dict(canvas=256, out_n=0), "out_n must be canvas, or 128 with canvas 256"),
        (dict(iters=0), "iters must be positive"),
        (dict(iters=-5), "iters must be positive"),
        (dict(traj=None), "null pointer"),
        (dict(fraction=None), "null pointer"),
        (dict(workspace=None), "null pointer"),
        (dict(B=-1), "null pointer"),
    ]
    for kwargs, text in refused:
        code, message = call(**kwargs)
        assert code == _lib.DIB_EINVAL, kwargs
        assert message == "dib_psf_rasterize: " + text, kwargs
    assert call(B=0)[0] == 0
    assert l.dib_psf_rasterize(None, 0, iters, None, 256, 1, 128, None, None, None, S) == 0
    assert l.dib_psf_rasterize_workspace_bytes(0, iters, 256) == 0
    torch.cuda.synchronize()
    for buf in (out64, out16, ws):
        assert bool((buf == SENTINEL).all())
    # the wrapper's own refusals
    with pytest.raises(TypeError, match="complex128"):
        blur_ops.rasterize_psfs(np.zeros((1, 4), np.complex64), [1.0], canvas=64)
    with pytest.raises(ValueError, match="one exposure fraction per trajectory"):
        blur_ops.rasterize_psfs(np.full((2, 4), 32 + 32j), [1.0], canvas=64)
    with pytest.raises(_lib.DibError, match="canvas must be 64, 128 or 256, got 100"):
        blur_ops.rasterize_psfs(np.full((1, 4), 32 + 32j), [1.0], canvas=100)
    # the same buffers then serve an accepted call
    assert call(canvas=256, out_n=256)[0] == 0
    torch.cuda.synchronize()
    want = O.psf_center(O.psf_rasterize(np.full(iters, 128.25), np.full(iters, 128.25), [0.5], 256)[0])
    assert np.array_equal(_bits(out64.cpu().numpy().view(np.float64).reshape(256, 256)), _bits(want))


def test_one_batch_call_captured_in_a_graph_replays_to_the_same_bytes():
    """The fractions travel in the kernel arguments (no copy to the device), so a captured call replays with them."""
    from detectinblur_amd import blur_ops
    case = BATCHES[2]
    name, canvas, traj, fracs = case
    dev = torch.from_numpy(traj).cuda()
    e64, e16 = blur_ops.rasterize_psfs(dev, fracs, canvas=canvas, center=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g64, g16 = blur_ops.rasterize_psfs(dev, fracs, canvas=canvas, center=True)
    g64.zero_()
    g16.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(g64.cpu().numpy()), _bits(e64.cpu().numpy()))
    assert np.array_equal(_bits(g16.cpu().numpy()), _bits(e16.cpu().numpy()))
    assert np.array_equal(_bits(g64.cpu().numpy()), _bits(RC.expected_batch(case)[1]))
