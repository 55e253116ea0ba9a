"""AugMix (reference transforms.py:68-79, augmix/augment_and_mix.py, augmix/augmentations.py), split into a plan and its application.

`draw_plan` makes exactly the reference's Python-`random`-free `np.random` draws, in its order (Dirichlet weights, Beta mix, the two
severities, then per chain its depth and per op the op and the op's own draws), and maps the boxes as the reference does.  The
plan is a small picklable dict:

    {"ws": (w0, w1, w2), "m": m, "chains": [[(op code, parameter), ...] x 3], "size": (H, W), "deferred": bool, "flip": bool}

`apply_plan` applies it on the host with the same Pillow operations the reference calls; `apply_plans_device` applies a batch of
plans on the GPU (csrc/dib_augmix.hip) and returns fp16 images equal bit for bit to `.half()` of the host path's result.  A plan
the loader leaves to the GPU ("deferred") records a later horizontal flip ("flip"): the image then arrives mirrored, and AugMix is
computed in the unflipped frame.
"""
import ctypes
import math

import numpy as np
import torch

# op codes: positions in the reference's `augmentations` list (include/dib.h DIB_AUGMIX_*)
AUTOCONTRAST, EQUALIZE, POSTERIZE, ROTATE, SOLARIZE, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y = range(9)
ALL_OPS = (AUTOCONTRAST, EQUALIZE, POSTERIZE, ROTATE, SOLARIZE, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y)
NON_POSITIONAL_OPS = (AUTOCONTRAST, EQUALIZE, POSTERIZE, SOLARIZE)
POSITIONAL_OPS = frozenset((ROTATE, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y))
OP_NAMES = ("autocontrast", "equalize", "posterize", "rotate", "solarize", "shear_x", "shear_y", "translate_x", "translate_y")
WIDTH, MAX_DEPTH = 3, 3
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)   # COCO constants of the reference's augment_and_mix.py


def _level(n):
    return np.random.uniform(low=0.1, high=n)


def _draw_op(op, severity, pos_severity, H, W):
    """The op's own draws (augmentations.py), in its order; returns its parameter."""
    if op == POSTERIZE:
        return 4 - int(_level(severity) * 4 / 10)
    if op == SOLARIZE:
        return 256 - int(_level(severity) * 256 / 10)
    if op == ROTATE:
        p = int(_level(pos_severity) * 30 / 10)
        return -p if np.random.uniform() > 0.5 else p
    if op in (SHEAR_X, SHEAR_Y):
        p = float(_level(pos_severity)) * 0.3 / 10.
        return -p if np.random.uniform() > 0.5 else p
    if op in (TRANSLATE_X, TRANSLATE_Y):
        p = int(_level(pos_severity) * (((W + H) / 2) / 3) / 10)
        return -p if np.random.random() > 0.5 else p
    return 0


def _map_boxes(boxes, op, p, H, W):
    """One positional op on the boxes, in place, as the reference does it: the four corners of each box (float32) through the
    op's map (float64 matrices for rotate / shear), then min / max, stored as float32."""
    if op == ROTATE:
        rad = -(p / 180) * np.pi
        mat = [[np.cos(rad), -np.sin(rad)], [np.sin(rad), np.cos(rad)]]
    elif op == SHEAR_X:
        mat = [[1, -p], [0, 1]]
    elif op == SHEAR_Y:
        mat = [[1, 0], [-p, 1]]
    for index, box in enumerate(boxes):
        b = box.numpy()
        pts = np.stack([np.array([b[0], b[1]]), np.array([b[2], b[1]]), np.array([b[0], b[3]]), np.array([b[2], b[3]])], axis=1)
        if op == ROTATE:
            pts[0, :] = pts[0, :] - W / 2
            pts[1, :] = pts[1, :] - H / 2
            pts = np.matmul(mat, pts)
            pts[0, :] = pts[0, :] + W / 2
            pts[1, :] = pts[1, :] + H / 2
        elif op in (SHEAR_X, SHEAR_Y):
            pts = np.matmul(mat, pts)
        elif op == TRANSLATE_X:
            pts[0, :] = pts[0, :] - p
        else:
            pts[1, :] = pts[1, :] - p
        boxes[index] = torch.tensor([pts[0, :].min(), pts[1, :].min(), pts[0, :].max(), pts[1, :].max()], dtype=torch.float32)


def _squeeze_boxes(boxes, H, W):
    """The reference's fix_bounding_box_squeeze (augment_and_mix.py:63-103): clamp to the image, widen empty boxes by one pixel on
    each side, clamp again."""
    def clamp():
        for col, lim in ((0, W - 1), (1, H - 1), (2, W - 1), (3, H - 1)):
            boxes[boxes[:, col] > lim, col] = lim
        for col in range(4):
            boxes[boxes[:, col] < 0, col] = 0
    clamp()
    for lo, hi in ((0, 2), (1, 3)):
        bad = boxes[:, lo] >= boxes[:, hi]
        boxes[bad, hi] = boxes[bad, hi] + 1
        boxes[bad, lo] = boxes[bad, lo] - 1
    clamp()
    return boxes


def draw_plan(H, W, positional=False, target=None, modify_target_boxes=False):
    """The reference's draws for one H x W image (augment_and_mix with severity = depth = -1, width 3, alpha 1).  Returns
    (plan, target): the target the reference returns -- a copy with the mapped, merged and clamped boxes when
    `modify_target_boxes`, else `target` itself."""
    ws = np.float32(np.random.dirichlet([1.] * WIDTH))
    m = np.float32(np.random.beta(1., 1.))
    severity = np.random.randint(1, 11)
    pos_severity = np.random.randint(1, 5)
    ops = ALL_OPS if positional else NON_POSITIONAL_OPS
    boxes = target["boxes"] if (modify_target_boxes and target is not None) else None
    chains, merged = [], None
    for _ in range(WIDTH):
        chain = []
        b = boxes.clone() if boxes is not None else None
        for _ in range(np.random.randint(1, 4)):
            op = ops[np.random.choice(len(ops))]
            p = _draw_op(op, severity, pos_severity, H, W)
            chain.append((op, p))
            if b is not None and op in POSITIONAL_OPS:
                _map_boxes(b, op, p, H, W)
        chains.append(chain)
        if b is not None:      # combine_targets: min of the top-left corners, max of the bottom-right ones
            merged = b if merged is None else torch.cat([torch.minimum(merged[:, :2], b[:, :2]), torch.maximum(merged[:, 2:], b[:, 2:])], 1)
    plan = {"ws": tuple(float(w) for w in ws), "m": float(m), "chains": chains, "size": (int(H), int(W)), "deferred": False,
            "flip": False}
    if merged is not None:
        target = dict(target)
        target["boxes"] = _squeeze_boxes(merged, H, W)
    return plan, target


# ---- host application ------------------------------------------------------------------------------------------------------

def _pil_op(im, op, p):
    from PIL import Image, ImageOps
    if op == AUTOCONTRAST:
        return ImageOps.autocontrast(im)
    if op == EQUALIZE:
        return ImageOps.equalize(im)
    if op == POSTERIZE:
        return ImageOps.posterize(im, p)
    if op == SOLARIZE:
        return ImageOps.solarize(im, p)
    if op == ROTATE:
        return im.rotate(p, resample=Image.BILINEAR)
    coeffs = {SHEAR_X: (1, p, 0, 0, 1, 0), SHEAR_Y: (1, 0, 0, p, 1, 0), TRANSLATE_X: (1, 0, p, 0, 1, 0), TRANSLATE_Y: (1, 0, 0, 0, 1, p)}[op]
    return im.transform(im.size, Image.AFFINE, coeffs, resample=Image.BILINEAR)


_NORM = None


def norm_table():
    """[3][256] float64: (k / 255 - mean_c) / std_c, numpy's value of the reference's normalize() at every uint8 level."""
    global _NORM
    if _NORM is None:
        k = np.arange(256) / 255
        _NORM = np.stack([(k - MEAN[c]) / STD[c] for c in range(3)])
    return _NORM


def apply_plan(img, plan):
    """H x W x 3 uint8 (unflipped) -> H x W x 3 uint8: the chains through Pillow, then the reference's float64 mix."""
    from PIL import Image
    N = norm_table()
    chan = np.arange(3)
    pil = Image.fromarray(np.ascontiguousarray(img))
    mix = np.zeros(img.shape, dtype=np.float64)
    for w, chain in zip(plan["ws"], plan["chains"]):
        im = pil
        for op, p in chain:
            im = _pil_op(im, op, p)
        mix += w * N[chan, np.asarray(im)]
    one_minus_m = float(np.float32(1) - np.float32(plan["m"]))     # (1 - m) is float32 in the reference
    mixed = one_minus_m * N[chan, img] + plan["m"] * mix
    mixed = mixed * np.asarray(STD) + np.asarray(MEAN)
    return (mixed * 255).astype(np.uint8)


def to_uint8_hwc(image):
    """What the reference's AugMix reads (np.asarray(image)): PIL / ndarray as they are; a float CHW tensor in [0, 1] (the synthetic
    dataset) as the uint8 image its PIL form holds."""
    if isinstance(image, torch.Tensor):
        return (image.permute(1, 2, 0).numpy() * 255).astype(np.uint8)
    return np.asarray(image)


def apply_deferred_host(image, plan):
    """A deferred plan on the host: float CHW image of k / 255 (mirrored when plan["flip"]) -> float CHW k / 255 of the AugMix
    result in the same frame (what the GPU path computes, before its fp16 rounding)."""
    img = torch.round(image.float() * 255).to(torch.uint8).permute(1, 2, 0).numpy()
    if plan["flip"]:
        img = img[:, ::-1]
    out = apply_plan(img, plan)
    if plan["flip"]:
        out = out[:, ::-1]
    return torch.from_numpy(np.ascontiguousarray(out.transpose(2, 0, 1))).to(torch.float32).div(255)


# ---- device application --------------------------------------------------------------------------------------------------------

def affine_coefficients(op, p, H, W):
    """Pillow's inverse affine coefficients of a positional op (Image.rotate's matrix, rounded to 15 decimals; an angle of 0 is a
    copy: the identity)."""
    if op == ROTATE:
        angle = p % 360.0
        if angle == 0:
            return (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
        cx, cy = W / 2, H / 2
        a = -math.radians(angle)
        m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
        m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
        m[2] += cx
        m[5] += cy
        return tuple(m)
    return tuple(float(v) for v in {SHEAR_X: (1, p, 0, 0, 1, 0), SHEAR_Y: (1, 0, 0, p, 1, 0), TRANSLATE_X: (1, 0, p, 0, 1, 0),
                                    TRANSLATE_Y: (1, 0, 0, 0, 1, p)}[op])


def plan_record(plan, src, dst, flip=None):
    """The plan as include/dib.h's dib_augmix_image for the 3 x H x W fp32 tensor `src` and fp16 tensor `dst`."""
    from . import _lib
    H, W = src.shape[-2], src.shape[-1]
    r = _lib.AugmixImage()
    r.src, r.dst, r.H, r.W = src.data_ptr(), dst.data_ptr(), H, W
    r.flip = int(plan["flip"] if flip is None else flip)
    for c, chain in enumerate(plan["chains"]):
        if len(chain) > MAX_DEPTH:
            raise ValueError("AugMix chain of %d ops (at most %d)" % (len(chain), MAX_DEPTH))
        r.n_ops[c] = len(chain)
        for j, (op, p) in enumerate(chain):
            r.op[c][j] = op
            if op in POSITIONAL_OPS:
                for k, v in enumerate(affine_coefficients(op, p, H, W)):
                    r.affine[c][j][k] = v
            else:
                r.iparam[c][j] = int(p)
    for c in range(WIDTH):
        r.ws[c] = plan["ws"][c]
    r.m = plan["m"]
    r.one_minus_m = float(np.float32(1) - np.float32(plan["m"]))
    return r


_CONSTS = {}


def _device_tables(device):
    t = _CONSTS.get(device)
    if t is None:
        norm = torch.from_numpy(norm_table().copy()).to(device)
        scale = torch.from_numpy(np.array([0.0] + [255.0 / d for d in range(1, 256)])).to(device)
        half = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255).half().view(torch.int16).to(device)
        t = _CONSTS[device] = (norm, scale, half)
    return t


def apply_plans_device(images, plans):
    """AugMix of a batch on the GPU: `images` are 3 x H x W fp32 CUDA tensors of k / 255 (mirrored when their plan says "flip"),
    one plan each.  Returns fp16 tensors, enqueued on the current stream (no host synchronisation)."""
    from . import _lib
    if not images:
        return []
    device = images[0].device
    if device.type != "cuda":
        raise ValueError("apply_plans_device needs CUDA tensors (apply_deferred_host is the host path)")
    n = len(images)
    srcs = [im.contiguous() if im.dtype == torch.float32 else im.float().contiguous() for im in images]
    for s in srcs:
        if s.dim() != 3 or s.shape[0] != 3:
            raise ValueError("AugMix images are 3 x H x W, got %s" % (tuple(s.shape),))
    outs = [torch.empty(s.shape, dtype=torch.float16, device=device) for s in srcs]
    l = _lib.lib()
    recs = (_lib.AugmixImage * n)()
    offset = 0
    for i, (s, o, plan) in enumerate(zip(srcs, outs, plans)):
        recs[i] = plan_record(plan, s, o)
        recs[i].buf_offset = offset
        offset += (l.dib_augmix_buffer_bytes(ctypes.byref(recs[i])) + 255) // 256 * 256
    nbytes = l.dib_augmix_workspace_bytes(n, offset)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)
    staged = torch.empty(ctypes.sizeof(recs), dtype=torch.uint8, pin_memory=True)
    ctypes.memmove(staged.data_ptr(), recs, ctypes.sizeof(recs))
    recs_dev = staged.to(device, non_blocking=True)
    norm, scale, half = _device_tables(device)
    _lib.check(l.dib_augmix(recs, recs_dev.data_ptr(), n, norm.data_ptr(), scale.data_ptr(), half.data_ptr(), workspace.data_ptr(),
                            nbytes, _lib.stream_of(workspace)))
    return outs
