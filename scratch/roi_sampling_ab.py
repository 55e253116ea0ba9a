"""The RoIAlign kernels of another build of libdib_hip.so (the parent commit's) against this tree's, on one MI355X: what
profiles/roi_sampling_isa.txt records below its table.

    python scratch/roi_sampling_ab.py PARENT_LIB            outputs, then timing
    python scratch/roi_sampling_ab.py PARENT_LIB outputs    forward of every kernel path on the seeded inputs of _general_cases()
                                                            (tests/test_roi_nms_reference.py): bit-identical or exit status 1
    python scratch/roi_sampling_ab.py PARENT_LIB time       device time per kernel at a training step's shapes

A process loads the library once (DIB_HIP_LIB), so every run of a build is a child process of its own; this process never
touches the GPU.  Timing: K = 4096 RoIs from _fpn_boxes (seed 0), C = 256, pooled 7, sampling ratio 2, the four levels of an
8-image 800 x 1344 batch (200 x 336 .. 25 x 42); device events around REPS calls after warm-up, the median per child; parent
and new children alternate, BLOCKS times.  The parent's spread is the range of its BLOCKS medians."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

REPS, BLOCKS, WARMUP = 20, 3, 3
K, C, P, SR = 4096, 256, 7, 2
LEVELS = [(200, 336), (100, 168), (50, 84), (25, 42)]
SCALES = [0.25, 0.125, 1.0 / 16, 1.0 / 32]


def child_outputs(path):
    from tests import test_roi_nms_reference as T
    out = {}
    for name, case in T._general_cases().items():
        feats, gout = T._general_inputs(case)
        got = T._run_kernels(feats, case["rois"], case["level"], case["scales"], gout, case["P"], case["sr"], case["aligned"])
        for k, (fwd, grads) in got.items():
            out["%s/%s/fwd" % (name, k)] = fwd
            for i, g in enumerate(grads):
                out["%s/%s/bwd%d" % (name, k, i)] = g
    np.savez(path, **out)


def child_time():
    import torch
    from detectinblur_amd import _lib
    from detectinblur_amd.models import detector_ops as ops
    from tests import test_roi_nms_reference as T
    dev = "cuda"
    rs = np.random.RandomState(0)
    boxes = T._fpn_boxes(rs, K, 800, 1344)
    rois = torch.tensor(np.concatenate([rs.randint(0, 8, (K, 1)).astype(np.float32), boxes], 1), device=dev)
    level = torch.tensor(T._fpn_level(boxes, 4), dtype=torch.int32, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    shapes = [(8, C, h, w) for h, w in LEVELS]
    cl = [T._cl(torch.randn(s, device=dev, generator=g)) for s in shapes]
    off = [T._misaligned_cl(x) for x in cl]                    # forces the generic channels-last forward
    planar = [x.contiguous() for x in cl]
    grads = [torch.zeros_like(x) for x in cl]                  # channels-last; the planar backward adds into the same bytes
    gout = torch.randn((K, C, P, P), device=dev, generator=g)
    out = torch.empty_like(gout)
    per_level = [torch.where(level == i)[0] for i in range(4)]
    r_lv = [rois[i].contiguous() for i in per_level]
    o_lv = [torch.empty((len(i), C, P, P), device=dev) for i in per_level]
    g_lv = [gout[i].contiguous() for i in per_level]
    hs, ws, sc = ops._level_arrays(shapes, SCALES)
    l, st = _lib.lib(), _lib.stream_of(out)

    def nhwc_fwd(xs):
        _lib.check(l.dib_roi_align_nhwc_forward(_lib.ptr_array([x.data_ptr() for x in xs]), hs, ws, sc, 4, rois.data_ptr(),
                                                level.data_ptr(), K, C, P, SR, 0, out.data_ptr(), st))

    def nhwc_bwd():
        _lib.check(l.dib_roi_align_nhwc_backward(gout.data_ptr(), hs, ws, sc, 4, rois.data_ptr(), level.data_ptr(), K, C, P, SR, 0,
                                                 _lib.ptr_array([x.data_ptr() for x in grads]), st))

    def planar_fwd():
        for i, (h, w) in enumerate(LEVELS):
            _lib.check(l.dib_roi_align_forward(planar[i].data_ptr(), r_lv[i].data_ptr(), len(r_lv[i]), C, h, w, SCALES[i], P, SR, 0,
                                               o_lv[i].data_ptr(), st))

    def planar_bwd():
        for i, (h, w) in enumerate(LEVELS):
            _lib.check(l.dib_roi_align_backward(g_lv[i].data_ptr(), r_lv[i].data_ptr(), len(r_lv[i]), C, h, w, SCALES[i], P, SR, 0,
                                                grads[i].data_ptr(), st))

    runs = [("roi_align_fwd_nhwc_sr_kernel<2>", lambda: nhwc_fwd(cl)), ("roi_align_fwd_nhwc_kernel", lambda: nhwc_fwd(off)),
            ("roi_align_bwd_nhwc_kernel", nhwc_bwd), ("roi_align_fwd_kernel (4 levels)", planar_fwd),
            ("roi_align_bwd_kernel (4 levels)", planar_bwd)]
    res = {}
    for name, fn in runs:
        for _ in range(WARMUP):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        res[name] = float(np.median([a.elapsed_time(b) for a, b in ev]))
    print("RESULT " + json.dumps(res))


def spawn(lib, *args):
    env = dict(os.environ)
    env.pop("DIB_HIP_LIB", None)
    if lib:
        env["DIB_HIP_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + list(args), env=env, capture_output=True, text=True)
    if p.returncode != 0:
        sys.exit("child (%s) failed with status %d:\n%s\n%s" % (lib or "this tree", p.returncode, p.stdout[-2000:], p.stderr[-4000:]))
    return p.stdout


def outputs(parent_lib):
    with tempfile.TemporaryDirectory() as d:
        a, b = os.path.join(d, "parent.npz"), os.path.join(d, "new.npz")
        spawn(parent_lib, "outputs", a)
        spawn(None, "outputs", b)
        old, new = np.load(a), np.load(b)
        assert sorted(old.files) == sorted(new.files)
        fwd = [k for k in old.files if k.endswith("/fwd")]
        bad = [k for k in fwd if not np.array_equal(old[k].view(np.uint32), new[k].view(np.uint32))]
        print("forward: %d outputs (%d elements) of %d cases, %d differ from the parent's in some bit" % (
            len(fwd), sum(old[k].size for k in fwd), len({k.split("/")[0] for k in fwd}), len(bad)))
        for k in bad:
            print("  DIFFERS", k, int((old[k].view(np.uint32) != new[k].view(np.uint32)).sum()), "elements")
        # the backward adds with atomics in an order that differs from run to run: reported, not held to anything here
        # (the exact-regime test holds it bit for bit where the sums are exact)
        worst = max(float(np.abs(old[k] - new[k]).max() / max(float(np.abs(old[k]).max()), 1e-30)) for k in old.files if "/bwd" in k)
        print("backward: largest |new - parent| / max|parent| over %d gradients: %.3g" % (sum("/bwd" in k for k in old.files), worst))
        return not bad


def timing(parent_lib):
    med = {"parent": [], "new": []}
    for _ in range(BLOCKS):
        for who, lib in (("parent", parent_lib), ("new", None)):
            line = [x for x in spawn(lib, "time").splitlines() if x.startswith("RESULT ")][-1]
            med[who].append(json.loads(line[7:]))
    print("device time in ms, median of %d calls per child, %d children per build (parent, new alternating)" % (REPS, BLOCKS))
    print("%-34s %-28s %-28s %8s %8s %8s  %s" % ("kernel", "parent", "new", "parent", "new", "spread", "new <= parent + spread"))
    ok = True
    for k in med["parent"][0]:
        a, b = [m[k] for m in med["parent"]], [m[k] for m in med["new"]]
        ma, mb, spread = float(np.median(a)), float(np.median(b)), max(a) - min(a)
        good = mb <= ma + spread
        ok = ok and good
        print("%-34s %-28s %-28s %8.4f %8.4f %8.4f  %s" % (k, " ".join("%.4f" % x for x in a), " ".join("%.4f" % x for x in b), ma, mb,
                                                           spread, "yes" if good else "NO"))
    return ok


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child_outputs(sys.argv[3]) if sys.argv[2] == "outputs" else child_time()
        sys.exit(0)
    parent_lib, what = os.path.abspath(sys.argv[1]), (sys.argv[2] if len(sys.argv) > 2 else "all")
    assert os.path.isfile(parent_lib), parent_lib
    ok = True
    if what in ("all", "outputs"):
        ok = outputs(parent_lib) and ok
    if what in ("all", "time"):
        ok = timing(parent_lib) and ok
    sys.exit(0 if ok else 1)
