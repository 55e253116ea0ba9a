"""Restoration quality on the GPU: the kernels of csrc/dib_quality.hip (dib_image_quality) against the float64 definition of
tests/test_quality.py -- the same pairs, the same tolerance rule max(8 d, 2^-20) with d the float32 restatement's own deviation, PSNR to
1e-3 dB -- at the tile's edges (the kernel's tile is 32 x 32 windows = 42 x 42 pixels), in all four dtype pairings, on views at odd element
offsets; the closed forms; determinism; what is written where; graph capture."""
import pytest
import torch

from tests.test_quality import KINDS, PAIRINGS, PSNR_TOL, case, check_against_reference, check_closed_forms

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TW = TH = 32          # csrc/dib_quality.hip: Q_TW, Q_TH
SHAPES = [(1, 11, 11), (3, 11, 75), (3, 75, 11), (3, 12, 12), (1, 10 + TH, 10 + TW), (1, 11 + TH, 11 + TW), (3, 37, 53), (3, 70, 90)]


def on_device(cs):
    return torch.from_numpy(cs["a"].copy()).to(DEV), torch.from_numpy(cs["b"].copy()).to(DEV)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_hip_against_the_float64_definition(shape, kind):
    from detectinblur_amd import quality as Q
    cs = case(kind, shape, "float16", "float32")
    a, b = on_device(cs)
    got = Q.psnr_ssim(a, b)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (3,)
    check_against_reference(got.tolist(), cs, "HIP %s %s" % (kind, shape))


@pytest.mark.parametrize("dt_a,dt_b", PAIRINGS)
@pytest.mark.parametrize("kind", KINDS)
def test_all_four_dtype_pairings_and_views_at_odd_element_offsets(kind, dt_a, dt_b):
    from detectinblur_amd import quality as Q
    shape = (3, 37, 53)
    cs = case(kind, shape, dt_a, dt_b)
    a, b = on_device(cs)
    got = Q.psnr_ssim(a, b)
    check_against_reference(got.tolist(), cs, "HIP %s %s/%s" % (kind, dt_a, dt_b))
    n = a.numel()
    views = []
    for t, off in ((a, 1), (b, 3)):           # the same values at an odd element offset of a larger buffer: element alignment only
        big = torch.zeros(n + 8, dtype=t.dtype, device=DEV)
        big[off:off + n] = t.flatten()
        views.append(big[off:off + n].view(shape))
        assert (views[-1].data_ptr() // t.element_size()) % 2 == 1 and views[-1].is_contiguous()
    assert torch.equal(Q.psnr_ssim(*views).view(torch.int32), got.view(torch.int32))


def test_a_full_size_half_pair():
    """3 x 800 x 1333: 3,150 workgroups, the last tile column 11 windows wide"""
    from detectinblur_amd import quality as Q
    cs = case("noise", (3, 800, 1333), "float16", "float16")
    a, b = on_device(cs)
    check_against_reference(Q.psnr_ssim(a, b).tolist(), cs, "HIP noise 3x800x1333 Half/Half")


def test_closed_forms_and_nan():
    from detectinblur_amd import quality as Q
    check_closed_forms(Q.psnr_ssim, DEV)


def test_two_calls_give_the_same_bytes():
    from detectinblur_amd import quality as Q
    for kind in KINDS:
        a, b = on_device(case(kind, (3, 70, 90), "float16", "float32"))
        first, second = Q.psnr_ssim(a, b), Q.psnr_ssim(a, b)
        assert torch.equal(first.view(torch.int32), second.view(torch.int32))


def test_only_the_result_and_the_stated_workspace_are_written():
    from detectinblur_amd import quality as Q
    shape = (3, 70, 90)
    a, b = on_device(case("smooth", shape, "float16", "float32"))
    need = Q.workspace_bytes(*shape)
    assert need == 3 * 2 * 3 * 16            # two doubles per workgroup; ceil(60 / 32) x ceil(80 / 32) tiles per plane
    SENT = -12345.0
    outbuf = torch.full((9,), SENT, dtype=torch.float32, device=DEV)
    workbuf = torch.full((need // 8 + 64,), SENT, dtype=torch.float64, device=DEV)
    work = workbuf[32:32 + need // 8]
    got = Q.psnr_ssim_hip(a, b, out=outbuf[3:6], work=work)
    assert got.data_ptr() == outbuf[3:6].data_ptr()
    assert (outbuf[:3] == SENT).all() and (outbuf[6:] == SENT).all() and (outbuf[3:6] != SENT).all()
    assert (workbuf[:32] == SENT).all() and (workbuf[32 + need // 8:] == SENT).all() and (work != SENT).all()
    assert torch.equal(got.view(torch.int32), Q.psnr_ssim(a, b).view(torch.int32))
    with pytest.raises(ValueError, match="work must hold"):
        Q.psnr_ssim_hip(a, b, work=workbuf[:need // 8 - 1])


def test_python_surface_on_the_device():
    from detectinblur_amd import _lib, quality as Q
    x = torch.rand(3, 20, 30, device=DEV)
    with pytest.raises(ValueError, match="smaller than"):
        Q.psnr_ssim(x[:, :10].contiguous(), x[:, :10].contiguous())
    with pytest.raises(ValueError, match="contiguous"):
        Q.psnr_ssim(x[:, :, ::2], x[:, :, ::2])
    with pytest.raises(ValueError, match="different devices"):
        Q.psnr_ssim(x, x.cpu())
    with pytest.raises(_lib.DibError, match="overlap"):          # the result inside an input
        Q.psnr_ssim_hip(x, x, out=x.view(-1)[:3])


def test_capturable():
    """two launches, no allocation inside the library, no synchronisation: the call replays from a HIP graph"""
    from detectinblur_amd import quality as Q
    cs = case("noise", (3, 37, 53), "float16", "float32")
    a, b = on_device(cs)
    out = torch.zeros(3, device=DEV)
    work = torch.empty(Q.workspace_bytes(3, 37, 53) // 8, dtype=torch.float64, device=DEV)
    want = Q.psnr_ssim_hip(a, b, work=work).clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        Q.psnr_ssim_hip(a, b, out=out, work=work)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
