"""Restoration quality (this repo; `train_deblurrer.py --validate_images`): how close an image is to the sharp one it was made from, as
mean squared error, PSNR and SSIM.  Where the blur runs on the device the sharp image is there right before the blur replaces it, so what
the blur took away and what a deblurrer or Richardson-Lucy (models/deblur.py, models/deconvolve.py) give back are measurable without
leaving the device.  `psnr_ssim` compares one pair and returns its three figures as a device tensor: nothing waits for the device.

The definition (include/dib.h, dib_image_quality; csrc/dib_quality.hip).  A stated reading -- DeepDeblur reports PSNR and SSIM, its loss/
package is not in the reference tree: Wang et al. 2004 as skimage.metrics.structural_similarity(gaussian_weights=True, sigma=1.5,
use_sample_covariance=False, data_range=L, channel_axis=0) computes it.  a, b: planar C x H x W, Half or fp32 each.
    mse = mean (a - b)^2;   psnr_db = 10 log10(L^2 / mse), +inf when mse == 0
    g: 11 taps, g_k ~ exp(-(k - 5)^2 / (2 1.5^2)), sum 1, separable;  every moment mu_a, mu_b, E[aa], E[bb], E[ab] is the VALID 11 x 11
    correlation with g (x) g: (H - 10) x (W - 10) windows per channel
    var_a = E[aa] - mu_a^2, var_b = E[bb] - mu_b^2, cov = E[ab] - mu_a mu_b;  C1 = (0.01 L)^2, C2 = (0.03 L)^2
    S = (2 mu_a mu_b + C1)(2 cov + C2) / ((mu_a^2 + mu_b^2 + C1)(var_a + var_b + C2));   ssim = mean of S over windows and channels
The kernel's arithmetic: pixels as fp32 minus a pivot that all pixels of a window share (today the mean of the 42 x 42 pixel tile a
workgroup stages: an implementation choice, not part of the contract; added back to the means), moments and S in fp32, the two means over the image in fp64; the window's fp32 weights are multiples of 2^-24 that sum to exactly 1
(WINDOW).

CUDA tensors take the HIP entry on the current stream (two launches, no synchronisation, workspace from torch's allocator: capturable);
CPU tensors take `psnr_ssim_torch`, the plain-torch restatement of the definition with the same window, in float64 (in float32 on
request: that form, shifted by L / 2, is what the HIP path's time is measured against on the GPU).

`restoration_quality(ref, candidates)` scores one or two candidates against one sharp image in one pass (include/dib.h,
dib_restoration_quality; csrc/dib_restoration.hip): the sharp image is read once, every candidate's figures are `psnr_ssim(candidate,
ref)` bit for bit, optionally on 8-bit grey levels, and an accumulator on the device takes the per-image figures in.
`RestorationMeter` is that accumulator for one sweep cell (`evaluate.py --restoration_metrics`): no read before `result()`.

No accuracy claim: PSNR and SSIM of synthetic images say how well a stage restores those images, nothing about detection AP."""
import math

import torch

TAPS = 11
HALO = TAPS - 1
# round(2^24 g_k) with the centre tap taking the residual: the eleven sum to 2^24 (csrc/dib_quality.hip holds the same integers)
_WINDOW_2_24 = (17253, 127486, 603993, 1834768, 3573640, 4462936, 3573640, 1834768, 603993, 127486, 17253)
assert sum(_WINDOW_2_24) == 1 << 24
WINDOW = tuple(v / float(1 << 24) for v in _WINDOW_2_24)


def _check(a, b, data_range):
    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float16, torch.float32):
            raise TypeError("psnr_ssim: %s must be a float16 or float32 tensor" % name)
        if t.dim() != 3:
            raise ValueError("psnr_ssim: %s must be planar C x H x W, got %s" % (name, tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("psnr_ssim: %s must be contiguous" % name)
    if a.shape != b.shape:
        raise ValueError("psnr_ssim: shapes differ: %s and %s" % (tuple(a.shape), tuple(b.shape)))
    if a.device != b.device:
        raise ValueError("psnr_ssim: the images are on different devices: %s and %s" % (a.device, b.device))
    if a.shape[0] < 1 or a.shape[1] < TAPS or a.shape[2] < TAPS:
        raise ValueError("psnr_ssim: image %s is smaller than the 11 x 11 window" % (tuple(a.shape),))
    L = float(data_range)
    if not (L > 0 and math.isfinite(L)):
        raise ValueError("psnr_ssim: data_range must be positive and finite, got %r" % (data_range,))
    return L


def _valid_correlation(q, dim):
    """sum_k g_k q[.., k : k + n] along `dim`, taps in order, in q's dtype"""
    n = q.shape[dim] - HALO
    acc = q.narrow(dim, 0, n) * WINDOW[0]
    for k in range(1, TAPS):
        acc = torch.add(acc, q.narrow(dim, k, n), alpha=WINDOW[k])
    return acc


@torch.no_grad()
def psnr_ssim_torch(a, b, data_range=1.0, out=None, dtype=torch.float64):
    """The definition in plain torch ops on the images' device (CPU or GPU): pixels minus L / 2 (added back to the means), moments and S
    in `dtype`, the two means over the image in float64.  No host synchronisation."""
    L = _check(a, b, data_range)
    half = 0.5 * L
    a32, b32 = a.to(dtype), b.to(dtype)
    d = a32 - b32
    mse = (d * d).double().mean()
    x, y = a32 - half, b32 - half
    m = _valid_correlation(_valid_correlation(torch.stack([x, y, x * x, y * y, x * y]), 3), 2)
    var_a, var_b, cov = m[2] - m[0] * m[0], m[3] - m[1] * m[1], m[4] - m[0] * m[1]
    mu_a, mu_b = m[0] + half, m[1] + half
    c1, c2 = _constants(L)
    S = ((2.0 * (mu_a * mu_b) + c1) * (2.0 * cov + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2))
    ssim = S.double().mean()
    psnr = 10.0 * torch.log10(L * L / mse)           # mse == 0: +inf; NaN: NaN
    res = torch.stack([mse, psnr, ssim]).float()
    if out is None:
        return res
    _check_out(out, a)
    out.copy_(res)
    return out


def _constants(L):
    """C1, C2 as the kernel forms them: fp32 products"""
    f = torch.tensor([0.01, 0.03], dtype=torch.float32) * torch.tensor(L, dtype=torch.float32)
    f = f * f
    return float(f[0]), float(f[1])


def _check_out(out, a):
    if out.dtype != torch.float32 or out.numel() != 3 or not out.is_contiguous() or out.device != a.device:
        raise ValueError("psnr_ssim: out must be 3 contiguous float32 elements on the images' device")


def workspace_bytes(C, H, W):
    from . import _lib
    return int(_lib.lib().dib_image_quality_workspace_bytes(int(C), int(H), int(W)))


@torch.no_grad()
def psnr_ssim_hip(a, b, data_range=1.0, out=None, work=None):
    """dib_image_quality on two CUDA images, on the current stream.  `work`: a CUDA byte tensor of at least workspace_bytes(C, H, W)
    bytes, 8-byte aligned (None: from torch's allocator)."""
    from . import _lib, blur_ops
    L = _check(a, b, data_range)
    if not a.is_cuda:
        raise TypeError("psnr_ssim_hip needs CUDA images")
    C, H, W = (int(v) for v in a.shape)
    if out is None:
        out = torch.empty(3, dtype=torch.float32, device=a.device)
    else:
        _check_out(out, a)
    need = workspace_bytes(C, H, W)
    if work is None:
        work = torch.empty(need // 8, dtype=torch.float64, device=a.device)
    elif work.numel() * work.element_size() < need or not work.is_contiguous() or work.device != a.device:
        raise ValueError("psnr_ssim_hip: work must hold %d contiguous bytes on the images' device" % need)
    _lib.check(_lib.lib().dib_image_quality(a.data_ptr(), blur_ops._DT[a.dtype], b.data_ptr(), blur_ops._DT[b.dtype], C, H, W, L,
                                            out.data_ptr(), work.data_ptr(), _lib.stream_of(a)))
    return out


ACC_DOUBLES = 6          # include/dib.h DIB_RQ_ACC_DOUBLES: n, n_identical, n_nonfinite, sum_mse, sum_psnr_db, sum_ssim
MAX_CANDIDATES = 2


def grey8(x):
    """the 8-bit grey levels of a [0, 1] image as fp32: round(clamp(255 x, 0, 255)), ties to even, a NaN stays a NaN -- what
    dib_restoration_quality does to every pixel it reads under quantize8"""
    return torch.round(torch.clamp(x.float() * 255, 0, 255))


def _check_restoration(ref, candidates, quantize, data_range):
    if isinstance(candidates, torch.Tensor):
        candidates = [candidates]
    candidates = list(candidates)
    if not 1 <= len(candidates) <= MAX_CANDIDATES:
        raise ValueError("restoration_quality: %d candidates, 1 or 2 are supported" % len(candidates))
    for c in candidates:
        L = _check(c, ref, data_range)
    if quantize and L != 1.0:
        raise ValueError("restoration_quality: quantize8 takes images in [0, 1]: data_range must be 1, got %r" % (data_range,))
    return candidates, L


def _check_buffers(out, acc, K, ref):
    if out is not None and (out.dtype != torch.float32 or out.numel() != 3 * K or not out.is_contiguous() or out.device != ref.device):
        raise ValueError("restoration_quality: out must be %d contiguous float32 elements on the images' device" % (3 * K))
    if acc is not None and (acc.dtype != torch.float64 or acc.numel() < ACC_DOUBLES * K or not acc.is_contiguous() or acc.device != ref.device):
        raise ValueError("restoration_quality: acc must be at least %d contiguous float64 elements on the images' device" % (ACC_DOUBLES * K))


def fold(acc_row, figures):
    """dib_restoration_quality's accumulator rule on the host: `figures` = (mse, psnr_db, ssim) as fp32 values, `acc_row` a list of
    ACC_DOUBLES floats, updated in place"""
    mse, psnr, ssim = (float(v) for v in figures)
    if not (math.isfinite(mse) and math.isfinite(ssim)):
        acc_row[2] += 1.0
        return acc_row
    acc_row[0] += 1.0
    acc_row[3] += mse
    acc_row[5] += ssim
    if mse == 0.0:
        acc_row[1] += 1.0
    else:
        acc_row[4] += psnr
    return acc_row


@torch.no_grad()
def restoration_quality_torch(ref, candidates, quantize8=False, data_range=1.0, out=None, acc=None):
    """the plain-torch form of restoration_quality: psnr_ssim_torch(candidate, ref) in float64 per candidate, on 8-bit grey levels with
    L = 255 under `quantize8`; the accumulator is folded on the host (this path reads its results)"""
    candidates, L = _check_restoration(ref, candidates, quantize8, data_range)
    K = len(candidates)
    _check_buffers(out, acc, K, ref)
    rows = [psnr_ssim_torch(grey8(c), grey8(ref), 255.0) if quantize8 else psnr_ssim_torch(c, ref, L) for c in candidates]
    res = torch.cat(rows)
    if acc is not None:
        host = acc.detach().cpu().tolist()
        for k, row in enumerate(rows):
            host[ACC_DOUBLES * k:ACC_DOUBLES * (k + 1)] = fold(host[ACC_DOUBLES * k:ACC_DOUBLES * (k + 1)], row.tolist())
        acc.copy_(torch.tensor(host, dtype=torch.float64))
    if out is None:
        return res
    out.copy_(res)
    return out


def restoration_workspace_bytes(K, C, H, W):
    from . import _lib
    return int(_lib.lib().dib_restoration_quality_workspace_bytes(int(K), int(C), int(H), int(W)))


@torch.no_grad()
def restoration_quality_hip(ref, candidates, quantize8=False, data_range=1.0, out=None, acc=None, work=None):
    """dib_restoration_quality on CUDA images, on the current stream: two launches whatever the number of candidates, nothing waits."""
    from . import _lib, blur_ops
    candidates, L = _check_restoration(ref, candidates, quantize8, data_range)
    if not ref.is_cuda:
        raise TypeError("restoration_quality_hip needs CUDA images")
    K = len(candidates)
    _check_buffers(out, acc, K, ref)
    C, H, W = (int(v) for v in ref.shape)
    if out is None:
        out = torch.empty(3 * K, dtype=torch.float32, device=ref.device)
    need = restoration_workspace_bytes(K, C, H, W)
    if work is None:
        work = torch.empty(need // 8, dtype=torch.float64, device=ref.device)
    elif work.numel() * work.element_size() < need or not work.is_contiguous() or work.device != ref.device:
        raise ValueError("restoration_quality_hip: work must hold %d contiguous bytes on the images' device" % need)
    _lib.check(_lib.lib().dib_restoration_quality(ref.data_ptr(), blur_ops._DT[ref.dtype], _lib.ptr_array([c.data_ptr() for c in candidates]),
                                                  _lib.int_array([blur_ops._DT[c.dtype] for c in candidates]), K, C, H, W, int(bool(quantize8)), L,
                                                  out.data_ptr(), None if acc is None else acc.data_ptr(), work.data_ptr(), _lib.stream_of(ref)))
    return out


def restoration_quality(ref, candidates, quantize8=False, data_range=1.0, out=None, acc=None, work=None):
    """ref: the sharp image; candidates: one or two images (a tensor or a sequence) to score against it; all planar C x H x W, contiguous,
    Half or fp32 in any mix, on one device.  Returns (or fills `out` with) 3 K fp32 elements: mse, psnr_db, ssim per candidate -- with
    quantize8 off exactly psnr_ssim(candidate, ref), bit for bit on the HIP path.  `quantize8`: every image is scored as its 8-bit grey
    levels (`grey8`), L = 255; data_range must be 1.  `acc`: ACC_DOUBLES float64 elements per candidate on the images' device,
    updated in place: n, n_identical (mse == 0: +inf dB, left out of the PSNR sum), n_nonfinite (NaN or infinite mse or ssim: counted,
    nothing added), sum_mse, sum_psnr_db, sum_ssim of the fp32 figures.  CUDA images take the HIP entry on the current stream (an error
    when the library is missing); CPU images the torch restatement."""
    if isinstance(ref, torch.Tensor) and ref.is_cuda:
        return restoration_quality_hip(ref, candidates, quantize8, data_range, out, acc, work)
    return restoration_quality_torch(ref, candidates, quantize8, data_range, out, acc)


class RestorationMeter(object):
    """One sweep cell's restoration figures (engine.evaluate(restoration_metrics=True)): per image the blurred one and, when a stage ran,
    the restored one against the sharp image, accumulated on the images' device.  Owns the accumulator, the workspace and the 3 K
    results; `update` queues two launches on the current stream and reads nothing; `result` makes the one device read of the cell."""

    def __init__(self, device, quantize8=False, names=("blurred", "restored")):
        if not 1 <= len(names) <= MAX_CANDIDATES:
            raise ValueError("RestorationMeter: %d names, 1 or 2 are supported" % len(names))
        self.device, self.quantize8, self.names = torch.device(device), bool(quantize8), tuple(names)
        self.acc = torch.zeros(ACC_DOUBLES * len(self.names), dtype=torch.float64, device=self.device)
        self.out = torch.zeros(3 * len(self.names), dtype=torch.float32, device=self.device)
        self.work, self.skipped = None, 0

    def reset(self):
        self.acc.zero_()
        self.skipped = 0

    def skip(self, n=1):
        """an image that was not blurred: nothing to compare"""
        self.skipped += int(n)

    def _workspace(self, shape):
        """sized for the largest image seen, for every name; regrown outside any capture (the old one goes back to torch's allocator,
        which keeps it until the launches queued on this stream are through)"""
        need = restoration_workspace_bytes(len(self.names), *shape)
        if self.work is None or self.work.numel() * 8 < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("RestorationMeter: the workspace has to grow for image %s; run one update of the largest image "
                                   "before capturing" % (tuple(shape),))
            self.work = torch.empty(need // 8, dtype=torch.float64, device=self.device)
        return self.work

    def update(self, sharp, blurred, restored=None):
        candidates = [blurred] if restored is None else [blurred, restored]
        if len(candidates) > len(self.names):
            raise ValueError("RestorationMeter: a restored image for a meter with names %s" % (self.names,))
        for c in candidates:
            if c.shape != sharp.shape:
                raise ValueError("RestorationMeter: image %s against a sharp image %s" % (tuple(c.shape), tuple(sharp.shape)))
        K = len(candidates)
        work = self._workspace(sharp.shape) if sharp.is_cuda else None
        return restoration_quality(sharp, candidates, self.quantize8, 1.0, self.out[:3 * K], self.acc[:ACC_DOUBLES * K], work)

    def result(self):
        """one device read, then -- with a process group up -- one all_reduce of the 6 K doubles and the skip count: a collective on
        every rank, whether its shard was empty or not"""
        import torch.distributed as dist
        t = torch.cat([self.acc.detach().cpu(), torch.tensor([float(self.skipped)], dtype=torch.float64)])
        if dist.is_available() and dist.is_initialized():
            t = t.to(self.device) if dist.get_backend() == "nccl" else t
            dist.all_reduce(t)
            t = t.cpu()
        v = t.tolist()
        L = 255.0 if self.quantize8 else 1.0
        nan = float("nan")
        res = {"skipped": int(v[-1]), "quantize8": self.quantize8}
        for k, name in enumerate(self.names):
            n, same, bad, s_mse, s_psnr, s_ssim = v[ACC_DOUBLES * k:ACC_DOUBLES * (k + 1)]
            mse = s_mse / n if n else nan
            res[name] = {"images": int(n), "identical": int(same), "nonfinite": int(bad), "mse": mse,
                         "psnr_db": s_psnr / (n - same) if n > same else nan,
                         "psnr_of_mean_mse_db": (float("inf") if mse == 0 else 10.0 * math.log10(L * L / mse)) if n else nan,
                         "ssim": s_ssim / n if n else nan}
        if len(self.names) == 2 and res[self.names[1]]["images"] > 0:
            a, b = res[self.names[0]], res[self.names[1]]
            res["psnr_gain_db"] = b["psnr_db"] - a["psnr_db"]
            res["ssim_gain"] = b["ssim"] - a["ssim"]
        return res


def format_restoration(res):
    """one line for a cell's `RestorationMeter.result()`"""
    parts = []
    for name, r in res.items():
        if isinstance(r, dict):
            parts.append("%s PSNR %.2f dB, SSIM %.4f (%d images%s%s)" % (name, r["psnr_db"], r["ssim"], r["images"],
                                                                       ", %d identical" % r["identical"] if r["identical"] else "",
                                                                       ", %d not finite" % r["nonfinite"] if r["nonfinite"] else ""))
    if "psnr_gain_db" in res:
        parts.append("gain %+.2f dB, %+.4f SSIM" % (res["psnr_gain_db"], res["ssim_gain"]))
    return "Restoration%s: %s; %d not blurred (no quality claim)" % (" (8-bit)" if res.get("quantize8") else "", "; ".join(parts), res["skipped"])


def psnr_ssim(a, b, data_range=1.0, out=None):
    """a, b: planar C x H x W, contiguous, Half or fp32 each, on one device.  Returns (or fills `out` with) 3 fp32 elements on that
    device: mse, psnr_db, ssim.  CUDA images take the HIP entry (an error when the library is missing: there is no fallback); CPU images
    the torch restatement.  ValueError: H or W < 11, shapes that differ, input that is not planar or not contiguous."""
    if isinstance(a, torch.Tensor) and a.is_cuda:
        return psnr_ssim_hip(a, b, data_range, out)
    return psnr_ssim_torch(a, b, data_range, out)
