"""`evaluate.py --deconvolve_first` (this repo): non-blind Richardson-Lucy deconvolution in front of the detector, with the blur's own
forward model.  In a synthetic pass the blur kernel is known exactly -- blur_dict["psf"], on the device already as the tap table the
blur has just read -- so this is the upper-bound companion of the paper's blind "deblur, then detect" baseline (models/deblur.py): what
deblurring could recover at all, given the true kernel.  It needs no weights.

The iteration (include/dib.h, dib_rl_deconvolve; csrc/dib_deconv.hip).  y: the image as the detector would get it (after the blur and
the corruptions), C x H x W, read as fp32.  Taps {(r_t, c_t, w_t)}: the normalised weights of the image's tap table in its row-major
order, not re-normalised.  K: the canvas (128 or 256), o = K / 2 - 1.
    (A  x)[i, j] = sum_t w_t x[m (i - (r_t - o)), m (j - (c_t - o))]      the blur itself: m = csrc/dib_common.h's map_coord with
                                                                          pad_mode_for(K, H, W), the wrap row / column included
    (A* u)[i, j] = sum_t w_t u[m'(i + (r_t - o)), m'(j + (c_t - o))]      m' = the same boundary rule without the wrap
    x_0 = y;  q = y / max(A x_k, eps);  x_{k+1} = clamp(x_k * A* q, 0, 1)
All in fp32; the result is fp32 C x H x W.  CUDA tensors take the HIP entry on the current stream (two launches per iteration, no
synchronisation, workspace from torch's allocator: capturable); CPU tensors take `richardson_lucy_torch`, the plain-torch restatement
(gathers by precomputed index vectors), which is also what the HIP path is measured against on the GPU.

No accuracy claim: synthetic data cannot show AP, and Richardson-Lucy amplifies whatever the forward model does not explain
(--add_noise, --add_jpeg_artefacts residue) a little more with every iteration: that is what --deconvolve_iterations is for.

The total-variation prior (`tv_lambda` > 0; evaluate.py --deconvolve_tv; Dey et al. 2006; include/dib.h, dib_tv_weight and
dib_rl_deconvolve_tv; csrc/dib_deconv_tv.hip) is the other remedy: one factor per pixel and iteration from a 7-point stencil of x_k,
    dx[i, j] = x[i, j + 1] - x[i, j] (0 in the last column)      dy[i, j] = x[i + 1, j] - x[i, j] (0 in the last row)
    n = sqrt(dx^2 + dy^2 + beta^2);  p = dx / n;  r = dy / n;  div[i, j] = (p[i, j] - p[i, j - 1]) + (r[i, j] - r[i - 1, j])
    g = 1 / (1 - lambda div);  x_{k+1} = clamp((x_k * g_k) * A* q, 0, 1)
which pulls the estimate toward piecewise-constant images: what A does not explain is no longer amplified iteration after iteration.
0 < lambda <= 0.1 (0.002 to 0.01 is the working range: larger values flatten detail), beta > 0 (1e-2: below that fp32 loses the
conditioning of dx / n on near-flat regions).  `tv_weight_torch` is the op-for-op restatement of x * g, `tv_weight` takes the HIP
entry for CUDA tensors (1 / n and g to 1 ulp there: the two agree to rounding); the HIP iteration is three launches and a 3-plane
workspace.  tv_lambda = 0 is the plain iteration, call for call."""
import math

import torch

PAD_REFLECT, PAD_ZERO, PAD_REPLICATE = 0, 1, 2
DEFAULT_ITERATIONS = 30
MAX_ITERATIONS = 1000
DEFAULT_TV_BETA = 1e-2
MAX_TV_LAMBDA = 0.1


def pad_mode_for(K, H, W):
    """csrc/dib_common.h: the padding of manual_blur by canvas and image size"""
    if K > 129:
        return PAD_REPLICATE
    return PAD_ZERO if (H < 64 or W < 64) else PAD_REFLECT


class Taps(object):
    """One PSF's taps on the host: rows, cols (int64) and fp32 weights in row-major order, and the canvas K."""

    def __init__(self, rows, cols, weights, K):
        self.rows, self.cols, self.weights, self.K = rows.long().cpu(), cols.long().cpu(), weights.float().cpu(), int(K)

    def __len__(self):
        return int(self.rows.numel())


def taps_of_psf(psf, normalize=True):
    """What the compaction writes for a K x K PSF: `psf / psf.sum()` in the PSF's own dtype (reference models/blur_functions.py:98), then
    its non-zero entries in row-major order."""
    psf = torch.as_tensor(psf)
    if psf.dim() != 2 or psf.shape[0] != psf.shape[1] or psf.shape[0] not in (128, 256):
        raise ValueError("PSF must be 128 x 128 or 256 x 256, got %s" % (tuple(psf.shape),))
    w = (psf / psf.sum() if normalize else psf).cpu()
    nz = w.nonzero()
    return Taps(nz[:, 0], nz[:, 1], w[nz[:, 0], nz[:, 1]], psf.shape[0])


def taps_of_table(tables, index=0):
    """The taps of table `index` of a blur_ops.TapTables, read back from the device (a copy to the host: tests and yardsticks only)."""
    rows, cols, bits = tables.taps(index)
    if getattr(tables, "dtype", torch.float16) == torch.float16:
        weights = (bits & 0xffff).to(torch.int16).view(torch.float16).float()
    else:
        weights = bits.to(torch.int32).view(torch.float32)
    return Taps(rows, cols, weights, tables.K)


def _as_taps(table_or_psf):
    if isinstance(table_or_psf, Taps):
        return table_or_psf
    if isinstance(table_or_psf, tuple):
        return taps_of_table(*table_or_psf)
    if hasattr(table_or_psf, "taps") and hasattr(table_or_psf, "buf"):
        return taps_of_table(table_or_psf, 0)
    return taps_of_psf(table_or_psf)


def _map(s, n, K, mode, wrap):
    """map_coord on a vector of virtual coordinates: (source index in [0, n), reads-zero mask)"""
    pa, pb = K // 2, K // 2 - 1
    if wrap:
        s = torch.where(s == -pa, torch.full_like(s, n + pb), s)
    zero = torch.zeros_like(s, dtype=torch.bool)
    if mode == PAD_REFLECT:
        s = torch.where(s < 0, -s, s)
        s = torch.where(s > n - 1, 2 * (n - 1) - s, s)
    elif mode == PAD_ZERO:
        zero = (s < 0) | (s > n - 1)
    return s.clamp(0, n - 1), zero


class _Sweeps(object):
    """The index vectors of A and A* for one (taps, H, W): per tap a row of H source rows and a row of W source columns, with their
    reads-zero masks folded into per-tap keep factors."""

    def __init__(self, taps, H, W, device):
        K, o = taps.K, taps.K // 2 - 1
        mode = pad_mode_for(K, H, W)
        i, j = torch.arange(H)[None, :], torch.arange(W)[None, :]
        dr, dc = (taps.rows - o)[:, None], (taps.cols - o)[:, None]
        self.weights = taps.weights.tolist()
        self.index = {}
        for adjoint in (False, True):
            ri, rz = _map(i + dr if adjoint else i - dr, H, K, mode, not adjoint)
            ci, cz = _map(j + dc if adjoint else j - dc, W, K, mode, not adjoint)
            keep = None
            if mode == PAD_ZERO:
                keep = ((~rz)[:, :, None] & (~cz)[:, None, :]).to(torch.float32).to(device)
            self.index[adjoint] = (ri.to(device), ci.to(device), keep)

    def apply(self, x, adjoint):
        ri, ci, keep = self.index[adjoint]
        acc = torch.zeros_like(x)
        for t, w in enumerate(self.weights):
            g = x.index_select(1, ri[t]).index_select(2, ci[t])
            if keep is not None:
                g = g * keep[t]
            acc = torch.add(acc, g, alpha=w)
        return acc


def _planar(image):
    if image.dim() == 2:
        return image[None]
    if image.dim() != 3:
        raise ValueError("image must be C x H x W (or H x W), got %s" % (tuple(image.shape),))
    return image


def _check(K, H, W, iterations, eps):
    if not (1 <= int(iterations) <= MAX_ITERATIONS):
        raise ValueError("richardson_lucy: iterations must lie in 1..%d, got %r" % (MAX_ITERATIONS, iterations))
    if not eps > 0:
        raise ValueError("richardson_lucy: eps must be positive, got %r" % (eps,))
    if K == 128 and not (H < 64 or W < 64) and (H == 64 or W == 64):
        raise RuntimeError("Padding size should be less than the corresponding input dimension (image is %dx%d): the blur refuses this "
                           "image, so its forward model is not defined" % (H, W))


def _check_tv(tv_lambda, tv_beta, who="richardson_lucy", needed=False):
    """True when the total-variation factor is on (tv_lambda > 0); 0 is the plain iteration unless the factor itself is asked for"""
    lam, beta = float(tv_lambda), float(tv_beta)
    if not ((0 < lam <= MAX_TV_LAMBDA) or (lam == 0 and not needed)):
        raise ValueError("%s: tv_lambda must lie in (0, %g]%s, got %r" % (who, MAX_TV_LAMBDA, "" if needed else " (or be 0: no prior)", tv_lambda))
    if not (beta > 0 and math.isfinite(beta)):
        raise ValueError("%s: tv_beta must be positive and finite, got %r" % (who, tv_beta))
    return lam > 0


def _f32(v):
    """the fp32 rounding of a Python number, as a Python float"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def _tv_weight(x, lam, b2):
    """x * g of fp32 planes C x H x W, every operation in the order of include/dib.h; lam, b2: fp32 values of lambda and beta * beta"""
    dx, dy = torch.zeros_like(x), torch.zeros_like(x)
    dx[:, :, :-1] = x[:, :, 1:] - x[:, :, :-1]
    dy[:, :-1, :] = x[:, 1:, :] - x[:, :-1, :]
    n = torch.sqrt(dx * dx + dy * dy + b2)
    p, r = dx / n, dy / n
    p_left, r_up = torch.zeros_like(x), torch.zeros_like(x)
    p_left[:, :, 1:] = p[:, :, :-1]
    r_up[:, 1:, :] = r[:, :-1, :]
    div = (p - p_left) + (r - r_up)
    return x * (1.0 / (1.0 - lam * div))


@torch.no_grad()
def tv_weight_torch(x, tv_lambda, tv_beta=DEFAULT_TV_BETA):
    """The total-variation factor applied: x * g (this module's docstring) in plain torch ops on x's device, fp32, of x's shape
    (C x H x W or H x W; planes independent)."""
    _check_tv(tv_lambda, tv_beta, "tv_weight", needed=True)
    b = _f32(tv_beta)
    return _tv_weight(_planar(x).float(), _f32(tv_lambda), _f32(b * b)).reshape(x.shape)


@torch.no_grad()
def tv_weight(x, tv_lambda, tv_beta=DEFAULT_TV_BETA):
    """x * g: CUDA tensors (Half or fp32) take dib_tv_weight on the current stream, one launch, no synchronisation; CPU tensors the
    torch restatement."""
    if not x.is_cuda:
        return tv_weight_torch(x, tv_lambda, tv_beta)
    from .. import _lib, blur_ops
    if x.dtype not in blur_ops._DT:
        raise TypeError("tv_weight needs a float16 / float32 image")
    _check_tv(tv_lambda, tv_beta, "tv_weight", needed=True)
    v = _planar(x)
    v = v if v.is_contiguous() else v.contiguous()
    C, H, W = (int(s) for s in v.shape)
    out = torch.empty((C, H, W), dtype=torch.float32, device=v.device)
    _lib.check(_lib.lib().dib_tv_weight(v.data_ptr(), blur_ops._DT[v.dtype], out.data_ptr(), C, H, W, float(tv_lambda), float(tv_beta),
                                        _lib.stream_of(v)))
    return out.reshape(x.shape)


def forward_blur(image, table_or_psf, adjoint=False):
    """A x (or A* x) in fp32 by the torch restatement, on the image's device."""
    taps = _as_taps(table_or_psf)
    x = _planar(image).float()
    out = _Sweeps(taps, x.shape[1], x.shape[2], x.device).apply(x, adjoint)
    return out.reshape(image.shape)


@torch.no_grad()
def richardson_lucy_torch(image, table_or_psf, iterations=DEFAULT_ITERATIONS, eps=1e-6, tv_lambda=0.0, tv_beta=DEFAULT_TV_BETA):
    """The iteration in plain torch ops on the image's device (CPU or GPU), fp32; tv_lambda > 0: with the total-variation factor."""
    taps = _as_taps(table_or_psf)
    y = _planar(image).float()
    _check(taps.K, y.shape[1], y.shape[2], iterations, eps)
    tv = _check_tv(tv_lambda, tv_beta)
    lam, b = _f32(tv_lambda), _f32(tv_beta)
    b2 = _f32(b * b)
    sweeps = _Sweeps(taps, y.shape[1], y.shape[2], y.device)
    x = y
    for _ in range(int(iterations)):
        q = y / sweeps.apply(x, False).clamp_min(eps)
        x = ((_tv_weight(x, lam, b2) if tv else x) * sweeps.apply(q, True)).clamp(0, 1)
    return x.reshape(image.shape)


@torch.no_grad()
def richardson_lucy_hip(image, tables, index=0, iterations=DEFAULT_ITERATIONS, eps=1e-6, tv_lambda=0.0, tv_beta=DEFAULT_TV_BETA):
    """dib_rl_deconvolve on a CUDA image with table `index` of a blur_ops.TapTables (compacted with normalize=True), on the current
    stream.  No synchronisation; the workspace (2 C H W floats) comes from torch's allocator.  tv_lambda > 0: dib_rl_deconvolve_tv,
    with a workspace of 3 C H W floats."""
    from .. import _lib, blur_ops
    if not image.is_cuda or image.dtype not in blur_ops._DT:
        raise TypeError("richardson_lucy_hip needs a float16 / float32 CUDA image")
    y = _planar(image)
    y = y if y.is_contiguous() else y.contiguous()
    C, H, W = (int(v) for v in y.shape)
    _check(tables.K, H, W, iterations, eps)
    tv = _check_tv(tv_lambda, tv_beta)
    if not 0 <= index < tables.count:
        raise ValueError("table index %d out of range (%d tables)" % (index, tables.count))
    blur_ops._await(tables)
    out = torch.empty((C, H, W), dtype=torch.float32, device=y.device)
    if tv:
        work = torch.empty((3, C, H, W), dtype=torch.float32, device=y.device)
        _lib.check(_lib.lib().dib_rl_deconvolve_tv(y.data_ptr(), blur_ops._DT[y.dtype], out.data_ptr(), work.data_ptr(), C, H, W,
                                                   tables.ptr(index), blur_ops._DT[getattr(tables, "dtype", torch.float16)], tables.K,
                                                   int(iterations), float(eps), float(tv_lambda), float(tv_beta), _lib.stream_of(y)))
        return out.reshape(image.shape)
    work = torch.empty((2, C, H, W), dtype=torch.float32, device=y.device)
    _lib.check(_lib.lib().dib_rl_deconvolve(y.data_ptr(), blur_ops._DT[y.dtype], out.data_ptr(), work.data_ptr(), C, H, W, tables.ptr(index),
                                            blur_ops._DT[getattr(tables, "dtype", torch.float16)], tables.K, int(iterations), float(eps),
                                            _lib.stream_of(y)))
    return out.reshape(image.shape)


def richardson_lucy(image, table_or_psf, iterations=DEFAULT_ITERATIONS, eps=1e-6, tv_lambda=0.0, tv_beta=DEFAULT_TV_BETA):
    """image: C x H x W (or H x W), Half or fp32, the blurred image.  table_or_psf: a blur_ops.TapTables (its first table), a
    (TapTables, index) pair, a K x K PSF tensor (un-normalised, as blur_dict["psf"]: divided by its sum in its own dtype, as the blur
    does) or a Taps.  Returns fp32 of the image's shape on its device.  CUDA images take the HIP entry (a PSF is compacted first); CPU
    images the torch restatement.  tv_lambda > 0 (and tv_beta): the total-variation factor in every iteration; 0: the plain iteration."""
    if not image.is_cuda:
        return richardson_lucy_torch(image, table_or_psf, iterations, eps, tv_lambda, tv_beta)
    from .. import blur_ops
    if isinstance(table_or_psf, tuple):
        tables, index = table_or_psf
    elif isinstance(table_or_psf, blur_ops.TapTables):
        tables, index = table_or_psf, 0
    elif isinstance(table_or_psf, Taps):
        raise TypeError("a CUDA image is deconvolved with a tap table or a PSF tensor (Taps live on the host: richardson_lucy_torch)")
    else:
        psf = torch.as_tensor(table_or_psf).to(image.device)
        tables, index = blur_ops.compact_psfs([psf], normalize=True), 0
    return richardson_lucy_hip(image, tables, index, iterations, eps, tv_lambda, tv_beta)


class Deconvolver(object):
    """The --deconvolve_first stage: `deconvolve_(image, blur_dict, psf, tables)` mirrors models.deblur.Deblurer.deblur_."""

    def __init__(self, iterations=DEFAULT_ITERATIONS, eps=1e-6, tv_lambda=0.0, tv_beta=DEFAULT_TV_BETA):
        if not (1 <= int(iterations) <= MAX_ITERATIONS):
            raise ValueError("Deconvolver: iterations must lie in 1..%d, got %r" % (MAX_ITERATIONS, iterations))
        if not eps > 0:
            raise ValueError("Deconvolver: eps must be positive, got %r" % (eps,))
        _check_tv(tv_lambda, tv_beta, "Deconvolver")
        self.iterations, self.eps = int(iterations), float(eps)
        self.tv_lambda, self.tv_beta = float(tv_lambda), float(tv_beta)      # 0: the plain iteration
        self.calls = 0

    def deconvolve_(self, image, blur_dict, psf, tables=None, index=0):
        """image: the blurred (and corrupted) image of a pass; blur_dict: its dictionary (an image with blurring == False is handed
        back untouched); psf: its un-normalised K x K PSF on the image's device; tables / index: the batch's staged tap tables and
        this image's table in them, or None -- mixed canvases, the library-owned path, the CPU -- and the stage compacts the PSF itself.
        Tables the blur had compacted for its large LDS window (a scheduling choice of blur_ops.large_window_pays) are not used
        either: the kernel would serve them, but in another tap order, and the result is not to depend on how the blur was scheduled."""
        if not blur_dict.get("blurring"):
            return image
        self.calls += 1
        if image.is_cuda and tables is not None and tables.K == psf.shape[0] and not tables.large:
            return richardson_lucy_hip(image, tables, index, self.iterations, self.eps, self.tv_lambda, self.tv_beta)
        return richardson_lucy(image, psf, self.iterations, self.eps, self.tv_lambda, self.tv_beta)
