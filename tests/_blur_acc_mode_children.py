"""Bodies of tests/test_blur_acc_mode_gpu.py's driver tests: each of the three `main()` functions with `--blur_acc_mode` in a
process of its own (the pattern of tests/_gpu_children.py, whose `_guarded` writes the result as JSON or the traceback to
`out_path + ".err"`).  A pass-through wrapper around every Python entry point that launches the blur notes what it was handed."""
import contextlib
import io
import math
import os
import sys

from tests._gpu_children import _guarded


class _FirstCell(Exception):
    pass


def _watch_blur_launches(seen):
    """blur_ops.sparse_blur (tables made ahead: the detector engines) and blur_ops.blur_step (library-owned tables: the estimator's
    engine, blur_image_list without `tables=`) pass through; per call the mode asked for and, where the caller owns the tables,
    whether they carry the vertical-run groups."""
    from detectinblur_amd import _lib, blur_ops
    real_sparse, real_step = blur_ops.sparse_blur, blur_ops.blur_step

    def sparse_blur(images, table_index, tables, acc_mode=_lib.DIB_ACC_BITEXACT):
        seen.append({"entry": "sparse_blur", "acc_mode": int(acc_mode), "vruns": bool(tables.vruns), "large": bool(tables.large), "K": int(tables.K)})
        return real_sparse(images, table_index, tables, acc_mode)

    def blur_step(images, table_index, psfs, normalize=True, acc_mode=_lib.DIB_ACC_BITEXACT, psfs_complete=False, large_window=False):
        seen.append({"entry": "blur_step", "acc_mode": int(acc_mode), "K": int(psfs[0].shape[0])})
        return real_step(images, table_index, psfs, normalize, acc_mode, psfs_complete, large_window)
    blur_ops.sparse_blur, blur_ops.blur_step = sparse_blur, blur_step


def _driver(which, argv):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    seen, out = [], {"losses": [], "stats": [], "accuracies": []}
    _watch_blur_launches(seen)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        if which == "train":
            from detectinblur_amd import train as M
            real_train, real_eval = M.train_one_epoch, M.evaluate

            def train_one_epoch(*a, **k):
                logger = real_train(*a, **k)
                out["losses"].append(float(logger.meters["loss"].global_avg))
                return logger

            def evaluate(*a, **k):
                ce = real_eval(*a, **k)
                out["stats"].append([float(x) for x in ce.coco_eval["bbox"].stats])
                return ce
            M.train_one_epoch, M.evaluate = train_one_epoch, evaluate
            M.main(M.build_parser().parse_args(list(argv)))
        elif which == "evaluate":
            from detectinblur_amd import evaluate as M
            real_eval = M.evaluate

            def evaluate(*a, **k):          # one sweep cell
                ce = real_eval(*a, **k)
                out["stats"].append([float(x) for x in ce.coco_eval["bbox"].stats])
                raise _FirstCell()
            M.evaluate = evaluate
            try:
                M.main(M.build_parser().parse_args(list(argv)))
            except _FirstCell:
                pass
        else:
            from detectinblur_amd import train_blur_estimator as M
            real_train, real_eval = M.train_one_epoch, M.evaluate

            def train_one_epoch(*a, **k):
                logger = real_train(*a, **k)
                out["losses"].append(float(logger.meters["loss"].global_avg))
                return logger

            def evaluate(*a, **k):
                acc = real_eval(*a, **k)
                out["accuracies"].append([float(x) for x in acc])
                return acc
            M.train_one_epoch, M.evaluate = train_one_epoch, evaluate
            M.main(M.build_parser().parse_args(list(argv)))
    out["calls"] = seen
    out["finite"] = all(math.isfinite(v) for group in (out["losses"], *out["stats"], *out["accuracies"]) for v in group)
    out["tail"] = buf.getvalue()[-600:]
    return out


def driver(out_path, which, argv):
    _guarded(_driver, out_path, (which, argv))
