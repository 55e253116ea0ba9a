"""Detection overlays: the picture the reference's `evaluate` saves of every image it scores (reference engine.py:382-383 around
utils.py:279-353) -- the image as the detector saw it, the outline of every detection above 0.5 drawn on it.

  * label_rgb          labels -> packed colours of the SAVED picture (the reference's colour handling, reproduced not fixed)
  * render_host        the numpy restatement of the pixel and outline rule of include/dib.h: the kernel's oracle, the CPU device's path
  * render_device      plan on the host, ONE launch of dib_overlay_rgb8 per 32 images, device uint8 tensors back
  * PngWriter          D2H into a ring of pinned slots on its own stream, PNG encoding on worker threads

The outline rule (include/dib.h) is a reading of cv2.rectangle(thickness=2); cv2 is not a dependency and the rule is
not pinned against it.
"""
import colorsys
import ctypes
import os
import threading

import numpy as np
import torch

COORD_MAX = 1 << 30          # box corners are clamped to +-2^30 (no image reaches that far; keeps the rule's +-2 inside int32)
SCORE_THRESHOLD = 0.5        # reference utils.py:342: `if score > 0.5`
MAX_LAUNCH = 32              # images per dib_overlay_rgb8 launch

# ---- colours ----------------------------------------------------------------------------------------------------------------------


def create_unique_color_float(tag, hue_step=0.05):
    """reference utils.py:279-300: an RGB colour per tag, in 0..255 floats (NOT bounded by 255: the channel gains exceed 1)."""
    h, v = (tag * hue_step) % 1, 1. - (int(tag * hue_step) % 4) / 5.
    r, g, b = colorsys.hsv_to_rgb(h, 1., v)
    r = (1 + ((tag % 10) / 1.5)) * r
    g = (1 + ((tag % 10) / 2)) * g
    b = (1 + ((tag % 10) / 3)) * b
    return r * 255, g * 255, b * 255


def compute_colors_for_labels(labels, palette=None):
    """reference utils.py:302-320: [n, 3] float64, create_unique_color_float(label) % 255 (`palette` is unused there too)."""
    colors = [create_unique_color_float(int(label)) for label in torch.as_tensor(labels).reshape(-1).tolist()]
    return np.asarray(colors) % 255


def _pack_rgb(color):
    """One colour tuple of compute_colors_for_labels -> R | G << 8 | B << 16 of the SAVED picture.  Two things happen to it in the
    reference, both kept: cv2 turns each float of the scalar into a byte by rounding half to even and saturating (cvRound +
    saturate_cast<uchar>), and the tuple (r, g, b) is drawn into a BGR array that is then converted BGR -> RGB (engine.py:383) -- in
    the saved picture red and blue are swapped."""
    b0, b1, b2 = (int(min(max(np.rint(c), 0), 255)) for c in color)          # np.rint: round half to even
    return b2 | b1 << 8 | b0 << 16


_TABLE = []          # packed colours of labels 0..90, built once per process


def label_rgb(labels):
    """labels (any integer sequence / tensor) -> list of packed colours (R | G << 8 | B << 16 of the saved picture)."""
    if not _TABLE:
        _TABLE.extend(_pack_rgb(c) for c in compute_colors_for_labels(list(range(91))))
    return [_TABLE[l] if 0 <= l < 91 else _pack_rgb(compute_colors_for_labels([l])[0]) for l in torch.as_tensor(labels).reshape(-1).tolist()]


# ---- the plan: which boxes, where, in which colour -------------------------------------------------------------------------------

def plan_boxes(boxes, labels, scores=None):
    """reference utils.py:334-351: the boxes with score > 0.5 (all of them without scores), corners truncated toward zero
    (`box.to(torch.int64)`) and clamped to +-2^30, in drawing order.  Returns an int64 array [n, 5]: x0, y0, x1, y1, packed colour."""
    boxes = torch.as_tensor(boxes).detach().cpu().reshape(-1, 4)
    labels = torch.as_tensor(labels).detach().cpu().reshape(-1)
    n = min(boxes.shape[0], labels.shape[0])                                 # zip() stops at the shortest
    if scores is not None:
        scores = torch.as_tensor(scores).detach().cpu().reshape(-1)
        n = min(n, scores.shape[0])
        keep = torch.nonzero(scores[:n] > SCORE_THRESHOLD).reshape(-1)
    else:
        keep = torch.arange(n)
    out = np.zeros((keep.numel(), 5), dtype=np.int64)
    if keep.numel():
        b = boxes[keep]
        if b.is_floating_point():
            b = torch.nan_to_num(b.double(), nan=0.0).clamp(-COORD_MAX, COORD_MAX)
        out[:, :4] = b.to(torch.int64).clamp(-COORD_MAX, COORD_MAX).numpy()
        out[:, 4] = label_rgb(labels[keep])
    return out


def _detection_plan(detection):
    return plan_boxes(detection["boxes"], detection["labels"], detection.get("scores"))


# ---- host restatement ---------------------------------------------------------------------------------------------------------------

def to_rgb8_host(image):
    """3 x H x W float / Half (tensor or array) -> H x W x 3 uint8: k = trunc(float32(x) * 255) saturated to 0..255, NaN -> 0."""
    a = image.detach().cpu().float().numpy() if isinstance(image, torch.Tensor) else np.asarray(image).astype(np.float32)
    with np.errstate(invalid="ignore"):
        v = a * np.float32(255.0)
        v = np.where(v >= 255.0, np.float32(255.0), np.where(v > 0.0, v, np.float32(0.0)))      # NaN fails both tests
    return np.ascontiguousarray(np.trunc(v).astype(np.uint8).transpose(1, 2, 0))


def draw_outline_host(rgb, x0, y0, x1, y1, packed):
    """The outline rule on an H x W x 3 array, in place: the four 3-pixel strips around the box's edges, clipped to the image, minus
    the four outermost corner pixels."""
    H, W = rgb.shape[:2]
    xa, xb, ya, yb = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
    color = np.array([packed & 255, packed >> 8 & 255, packed >> 16 & 255], dtype=np.uint8)
    corners = [(y, x) for y in (ya - 1, yb + 1) for x in (xa - 1, xb + 1) if 0 <= y < H and 0 <= x < W]
    kept = [rgb[y, x].copy() for y, x in corners]
    X0, X1, Y0, Y1 = max(xa - 1, 0), min(xb + 1, W - 1), max(ya - 1, 0), min(yb + 1, H - 1)
    if X0 > X1 or Y0 > Y1:
        return
    for lo, hi in ((ya - 1, ya + 1), (yb - 1, yb + 1)):              # horizontal edges
        lo, hi = max(lo, Y0), min(hi, Y1)
        if lo <= hi:
            rgb[lo:hi + 1, X0:X1 + 1] = color
    for lo, hi in ((xa - 1, xa + 1), (xb - 1, xb + 1)):              # vertical edges
        lo, hi = max(lo, X0), min(hi, X1)
        if lo <= hi:
            rgb[Y0:Y1 + 1, lo:hi + 1] = color
    for (y, x), old in zip(corners, kept):
        rgb[y, x] = old


def render_host(image, boxes, labels, scores=None):
    """The saved picture of one image, on the host: H x W x 3 uint8 RGB.  `image`: 3 x H x W float or Half; `boxes` [n, 4], `labels`
    [n], `scores` [n] or None (then every box is drawn, as in the reference)."""
    rgb = to_rgb8_host(image)
    for x0, y0, x1, y1, packed in plan_boxes(boxes, labels, scores).tolist():
        draw_outline_host(rgb, x0, y0, x1, y1, packed)
    return rgb


# ---- device ---------------------------------------------------------------------------------------------------------------------------

def render_device(images, detections, stream=None):
    """The saved pictures of a list of CUDA images (3 x H x W, Half or float32, one dtype per call) as device uint8 tensors
    [H, W, 3].  `detections`: per image a dict of CPU tensors (boxes, labels, optionally scores).  The plan is built on the host,
    uploaded from one pinned block and drawn by one launch per 32 images, all on `stream` (a torch.cuda.Stream; default: the
    current one).  No host synchronisation."""
    from . import _lib
    if len(images) != len(detections):
        raise ValueError("render_device: %d images, %d detections" % (len(images), len(detections)))
    if not images:
        return []
    dtype = images[0].dtype
    if dtype not in (torch.float16, torch.float32):
        raise TypeError("render_device: images must be Half or float32, got %s" % dtype)
    for im in images:
        if not (im.is_cuda and im.dim() == 3 and im.shape[0] == 3 and im.dtype == dtype and im.device == images[0].device):
            raise ValueError("render_device: every image must be a 3 x H x W CUDA tensor of one dtype on one device")
    plans = [_detection_plan(d) for d in detections]
    device = images[0].device
    with torch.cuda.device(device), torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(device)):
        raw = _lib.stream_of(images[0])
        images = [im.contiguous() for im in images]
        total = sum(p.shape[0] for p in plans)
        boxes_dev = None
        if total:
            host = torch.empty((total, 5), dtype=torch.int32, pin_memory=True)
            rows = np.concatenate(plans, axis=0)
            rows[:, 4] &= 0xffffff
            host.copy_(torch.from_numpy(rows.astype(np.int32)))
            boxes_dev = host.to(device, non_blocking=True)
        outs = [torch.empty((im.shape[1], im.shape[2], 3), dtype=torch.uint8, device=device) for im in images]
        offsets = np.concatenate([[0], np.cumsum([p.shape[0] for p in plans])]).astype(np.int64).tolist()
        for lo in range(0, len(images), MAX_LAUNCH):
            hi = min(lo + MAX_LAUNCH, len(images))
            _lib.check(_lib.lib().dib_overlay_rgb8(
                _lib.ptr_array([im.data_ptr() for im in images[lo:hi]]), _lib.DIB_F16 if dtype == torch.float16 else _lib.DIB_F32,
                _lib.int_array([im.shape[1] for im in images[lo:hi]]), _lib.int_array([im.shape[2] for im in images[lo:hi]]), hi - lo,
                ctypes.c_void_p(boxes_dev.data_ptr() if boxes_dev is not None else None), _lib.int_array(offsets[lo:hi + 1]),
                _lib.ptr_array([o.data_ptr() for o in outs[lo:hi]]), ctypes.c_void_p(raw)))
    return outs


# ---- PNG files ------------------------------------------------------------------------------------------------------------------------

def save_png(path, rgb):
    """H x W x 3 uint8 RGB -> a PNG file, the reference's way (engine.py:383: PIL, default settings)."""
    from PIL import Image
    Image.fromarray(rgb).save(path)


class PngWriter(object):
    """Writes `<folder>/img<count>.png` without holding the evaluation loop up.  `submit(count, rgb)` queues the device-to-host copy
    of an [H, W, 3] uint8 CUDA tensor into one of `depth` pinned slots on the writer's own stream, records an event behind it and
    hands (slot, event, file name) to a pool of `workers` threads; a worker waits for ITS event (never for the device), encodes the
    PNG and frees the slot.  A full ring blocks `submit`: back-pressure, and at most `depth` pictures of pinned memory.  A host
    array / CPU tensor goes to the pool as it is.  `close()` drains the pool and re-raises the first error a worker hit.  The folder
    is created if missing (the reference crashes there)."""

    def __init__(self, folder, workers=4, depth=8):
        from concurrent.futures import ThreadPoolExecutor
        self.folder = str(folder)
        os.makedirs(self.folder, exist_ok=True)
        self.depth = int(depth)
        self._pool = ThreadPoolExecutor(max_workers=int(workers), thread_name_prefix="dib_png")
        self._free = threading.Semaphore(self.depth)
        self._lock = threading.Lock()
        self._idle = list(range(self.depth))
        self._slots = [None] * self.depth           # pinned uint8 buffers, grown to the largest picture seen
        self._futures = []
        self._stream = None
        self._closed = False

    def path(self, count):
        return os.path.join(self.folder, "img" + str(count) + ".png")

    def stream(self, device):
        """The writer's stream on `device` (the render of a picture is queued there too: engine.evaluate)."""
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=device)
        return self._stream

    def _work(self, slot, event, path, array):
        try:
            if event is not None:
                event.synchronize()
            save_png(path, array)
        finally:
            with self._lock:
                self._idle.append(slot)
            self._free.release()

    def submit(self, count, rgb):
        if self._closed:
            raise RuntimeError("PngWriter.submit after close()")
        self._free.acquire()                            # blocks while every slot is on its way to a file
        with self._lock:
            slot = self._idle.pop()
        try:
            event = None
            if isinstance(rgb, torch.Tensor) and rgb.is_cuda:
                stream = self.stream(rgb.device)
                n = rgb.numel()
                if self._slots[slot] is None or self._slots[slot].numel() < n:
                    self._slots[slot] = torch.empty((n,), dtype=torch.uint8, pin_memory=True)
                view = self._slots[slot][:n].view(rgb.shape)
                producer = torch.cuda.current_stream(rgb.device)
                if producer != stream:                   # a picture rendered elsewhere: the copy goes behind what is queued there
                    stream.wait_stream(producer)
                with torch.cuda.stream(stream):
                    view.copy_(rgb, non_blocking=True)
                    event = torch.cuda.Event()
                    event.record(stream)
                rgb.record_stream(stream)
                array = view.numpy()
            else:
                array = rgb.numpy() if isinstance(rgb, torch.Tensor) else np.asarray(rgb)
            if len(self._futures) >= 8 * self.depth:      # keep what is pending or failed, forget the rest
                self._futures = [f for f in self._futures if not f.done() or f.exception() is not None]
            self._futures.append(self._pool.submit(self._work, slot, event, self.path(count), array))
        except BaseException:
            with self._lock:
                self._idle.append(slot)
            self._free.release()
            raise

    def close(self):
        """Waits for every picture on its way; re-raises the first error a worker hit.  Idempotent."""
        if self._closed:
            return
        self._closed = True
        self._pool.shutdown(wait=True)
        futures, self._futures = self._futures, []
        self._slots = [None] * self.depth
        for f in futures:
            f.result()


class EvaluationPictures(object):
    """The pictures of one pass of engine.evaluate (`image_output_folder`; None: no picture, no writer): a PngWriter on the folder
    -- with more than one rank on `<folder>/rank<r>/` (the reference lets the ranks overwrite each other) -- fed by the loop in two
    steps, `take` where the image is complete and `save` where its detections have arrived."""

    def __init__(self, image_output_folder):
        from . import utils
        self.writer = None
        if image_output_folder is not None:
            folder = str(image_output_folder)
            if utils.get_world_size() > 1:
                folder = os.path.join(folder, "rank%d" % utils.get_rank())
            self.writer = PngWriter(folder)

    def take(self, images, index):
        """What `save` needs for image `index`'s picture: the first image of the batch as it stands now (the caller has just
        synchronised: it is complete), an event that says so to the writer's stream, and the loop's index."""
        if self.writer is None:
            return None
        image, complete = images[0], None
        if image.is_cuda:
            complete = torch.cuda.Event()
            complete.record()
        return image, complete, index

    def save(self, picture, output):
        image, complete, index = picture
        if not image.is_cuda:
            save_png(self.writer.path(index), render_host(image, output["boxes"], output["labels"], output.get("scores")))
            return
        # render and copy on the writer's stream, behind the event; nothing here waits for the device (a full ring of
        # pictures still being encoded does hold the loop: PngWriter.submit)
        stream = self.writer.stream(image.device)
        stream.wait_event(complete)
        image.record_stream(stream)
        with torch.cuda.stream(stream):
            self.writer.submit(index, render_device([image], [output], stream=stream)[0])

    def close(self):
        """`evaluate`'s `finally`: drains the encoders; re-raises the first error one of them hit"""
        if self.writer is not None:
            self.writer.close()
