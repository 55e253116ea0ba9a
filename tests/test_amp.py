"""`--amp` (bfloat16 trunk) without a GPU: the flag, the dtype contract of `compute_dtype=torch.bfloat16` on plain torch ops,
checkpoints both ways, DDP over gloo, the two drivers end to end on toy sizes, and the new kernels' resource report.
Every test here fails on a tree without the flag."""
import contextlib
import io
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _small_model(compute_dtype=torch.float32):
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    torch.manual_seed(0)
    return fasterrcnn_resnet50_fpn(pretrained=False, pretrained_backbone=False, num_classes=91, min_size=96, max_size=128,
                                   rpn_pre_nms_top_n_train=200, rpn_post_nms_top_n_train=100, rpn_post_nms_top_n_test=50,
                                   box_batch_size_per_image=32, compute_dtype=compute_dtype)


def _batch():
    g = torch.Generator().manual_seed(3)
    imgs = [torch.rand(3, 90, 120, generator=g), torch.rand(3, 96, 100, generator=g)]
    tg = [{"boxes": torch.tensor([[10., 20., 60., 70.]]), "labels": torch.tensor([3])},
          {"boxes": torch.tensor([[5., 5., 50., 60.], [20., 30., 90., 80.]]), "labels": torch.tensor([1, 9])}]
    return imgs, tg


def test_both_parsers_accept_amp_and_refuse_it_with_mode_one_norm():
    from detectinblur_amd import evaluate, train
    for mod in (train, evaluate):
        on = mod.build_parser().parse_args(["--synthetic", "--amp"])
        off = mod.build_parser().parse_args(["--synthetic"])
        assert on.amp is True and off.amp is False
        train.reject_out_of_scope(on)                                 # passes
        assert train.detector_size_kwargs(on) == {"compute_dtype": torch.bfloat16} and train.detector_size_kwargs(off) == {}
        assert "amp=True" in str(on)                                  # what print(args) shows
    help_text = " ".join(train.build_parser().format_help().split())      # argparse wraps the lines
    assert "bfloat16" in help_text and "fp32 master weights" in help_text
    both = evaluate.build_parser().parse_args(["--synthetic", "--amp", "--mode_one_norm"])
    with pytest.raises(SystemExit) as e:
        train.reject_out_of_scope(both)
    assert "--amp" in str(e.value) and "--mode_one_norm" in str(e.value)
    with pytest.raises(SystemExit) as e:
        evaluate.main(both)
    assert "--amp" in str(e.value) and "--mode_one_norm" in str(e.value)
    with pytest.raises(ValueError):
        _small_model(torch.float16)


def test_dtype_contract_and_checkpoints_both_ways(tmp_path):
    amp, ref = _small_model(torch.bfloat16), _small_model()
    assert amp.backbone.compute_dtype == torch.bfloat16 and ref.backbone.compute_dtype == torch.float32
    sd_amp, sd_ref = amp.state_dict(), ref.state_dict()
    assert list(sd_amp) == list(sd_ref)
    assert all(sd_amp[k].dtype == sd_ref[k].dtype and sd_amp[k].shape == sd_ref[k].shape for k in sd_ref)
    assert all(v.dtype == torch.float32 for v in sd_amp.values() if v.is_floating_point())
    # activations: bf16 inside the body, fp32 levels out, the bf16 level each was upcast from travelling with it
    seen = []
    h = amp.backbone.body.layer2.register_forward_hook(lambda mod, i, o: seen.append((i[0].dtype, o.dtype)))
    amp.train()
    x = torch.rand(2, 3, 96, 128).contiguous(memory_format=torch.channels_last)
    levels = amp.backbone(x)
    assert seen == [(torch.bfloat16, torch.bfloat16)]
    assert list(levels) == ["0", "1", "2", "3", "pool"]
    for v in levels.values():
        assert v.dtype == torch.float32 and v._dib_lp.dtype == torch.bfloat16 and torch.equal(v, v._dib_lp.float())
    h.remove()
    # the fp32 model's levels are close (same weights: same seed), not equal: the mode really computes in bf16
    ref.train()
    want = ref.backbone(x)
    for k in want:
        err = float((levels[k] - want[k]).abs().max() / want[k].abs().max())
        assert 0 < err < 0.1, (k, err)
    # a training step: finite losses, every parameter and gradient fp32
    imgs, tg = _batch()
    losses = amp(imgs, tg)
    assert set(losses) == {"loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg"}
    assert all(v.dtype == torch.float32 and torch.isfinite(v) for v in losses.values())
    sum(losses.values()).backward()
    for n, p in amp.named_parameters():
        assert p.dtype == torch.float32 and p.grad is not None and p.grad.dtype == torch.float32, n
        assert torch.isfinite(p.grad).all(), n
    assert float(amp.backbone.body.layer1[0].conv1.weight.grad.abs().sum()) > 0
    assert float(amp.backbone.fpn.inner_blocks[0].bias.grad.abs().sum()) > 0
    # save under amp -> load without, and back
    torch.save({"model": amp.state_dict()}, tmp_path / "amp.pth")
    ref.load_state_dict(torch.load(tmp_path / "amp.pth", weights_only=True)["model"], strict=True)
    torch.save({"model": ref.state_dict()}, tmp_path / "ref.pth")
    amp.load_state_dict(torch.load(tmp_path / "ref.pth", weights_only=True)["model"], strict=True)
    assert amp.backbone.compute_dtype == torch.bfloat16               # not part of the state
    # inference: detections come out, the cached bf16 folds follow a weight update
    amp.eval()
    with torch.no_grad():
        det = amp(imgs)
        assert len(det) == 2 and all(d["boxes"].dtype == torch.float32 for d in det)
        conv = amp.backbone.body.layer1[0].conv2
        from detectinblur_amd.models import backbone as B
        w_lp, shift = B._folded(conv, amp.backbone.body.layer1[0].bn2, torch.bfloat16)
        assert w_lp.dtype == torch.bfloat16 and shift.dtype == torch.float32
        ptr = w_lp.data_ptr()
        conv.weight.mul_(2.0)
        assert B.refresh_folded(amp.backbone) >= 1
        again, _ = B._folded(conv, amp.backbone.body.layer1[0].bn2, torch.bfloat16)
        assert again.data_ptr() == ptr                                # rewritten in place: a captured graph keeps reading it
        w32, _ = B._folded(conv, amp.backbone.body.layer1[0].bn2)
        assert torch.equal(again, w32.to(torch.bfloat16))


def test_amp_with_warp_in_model_cpu():
    """`--amp --warp_in_model`: the warper sees fp32 on both sides of the bf16 trunk (the un-stretched levels are new fp32 tensors, so
    the RPN head runs in fp32 on them); with killWarp the head reads the bf16 levels."""
    from detectinblur_amd.models.faster_rcnn import fasterrcnn_resnet50_fpn
    torch.manual_seed(0)
    # the model, batch and warp parameters of tests/test_warper.py::test_detector_forward_with_warp_in_model_cpu
    m = fasterrcnn_resnet50_fpn(num_classes=5, pretrained=False, pretrained_backbone=False, warp_internally=True, channels_last=False,
                                min_size=96, max_size=128, compute_dtype=torch.bfloat16)
    m.train()
    seen = []
    m.warper.register_forward_hook(lambda mod, i, o: seen.append((i[0].dtype, o.dtype)))
    imgs = [torch.rand(3, 96, 128), torch.rand(3, 90, 120)]
    tg = [{"boxes": torch.tensor([[10.0, 12, 60, 70]]), "labels": torch.tensor([2])},
          {"boxes": torch.tensor([[5.0, 8, 40, 44], [30, 30, 80, 85]]), "labels": torch.tensor([1, 3])}]
    th, l1, l2 = torch.tensor([0.4, -0.2]).half(), torch.tensor([0.9, 0.85]).half(), torch.tensor([1.0, 0.97]).half()
    losses = m(imgs, tg, thetas=th, lambda1s=l1, lambda2s=l2)
    assert all(torch.isfinite(v) and v.dtype == torch.float32 for v in losses.values())
    assert len(seen) == 6 and all(a == torch.float32 and b == torch.float32 for a, b in seen)
    sum(losses.values()).backward()
    assert all(p.grad is not None and p.grad.dtype == torch.float32 for p in m.backbone.parameters())
    unwarped = m(imgs, tg, thetas=th, lambda1s=l1, lambda2s=l2, killWarp=True)
    assert all(torch.isfinite(v) for v in unwarped.values()) and len(seen) == 6


def test_plain_torch_epilogues_keep_the_bf16_storage_contract():
    """The plain-torch forms (CPU; GPU with the switches off) compute in fp32 and round once: the expressions the kernels are
    held to bit for bit in tests/test_amp_gpu.py."""
    from detectinblur_amd.models import backbone as B
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 16, 5, 7, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    r = torch.randn(2, 16, 5, 7, generator=g).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    bias = torch.randn(16, generator=g)
    y = B.bias_act(x.clone(), bias, r, relu=True)
    assert y.dtype == torch.bfloat16
    assert torch.equal(y, torch.relu(x.float() + bias.reshape(1, -1, 1, 1) + r.float()).to(torch.bfloat16))
    top = torch.randn(2, 16, 3, 4, generator=g).to(torch.bfloat16)
    m = B.topdown_merge(x.clone(), bias, top)
    assert m.dtype == torch.bfloat16
    up = torch.nn.functional.interpolate(top.float(), size=(5, 7), mode="nearest")
    assert torch.equal(m, ((x.float() + bias.reshape(1, -1, 1, 1)) + up).to(torch.bfloat16))


_DDP_SCRIPT = r'''
import copy, os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
from detectinblur_amd import utils
from tests.test_amp import _small_model
from tests.test_engine_ddp_cpu import _rank_batch
class A: pass
args = A(); args.dist_url = "env://"
utils.init_distributed_mode(args)
assert args.distributed and args.dist_backend == "gloo" and dist.get_world_size() == 2
rank = dist.get_rank()
m = _small_model(torch.bfloat16)
bare = copy.deepcopy(m)
assert bare.backbone.compute_dtype == torch.bfloat16
ddp = torch.nn.parallel.DistributedDataParallel(m, broadcast_buffers=False, gradient_as_bucket_view=True)
ddp.train(); bare.train()
seen = []
m.backbone.body.layer3.register_forward_hook(lambda mod, i, o: seen.append(o.dtype))
imgs, tg = _rank_batch(rank, 0)
torch.manual_seed(5)
sum(ddp(imgs, tg).values()).backward()
assert seen == [torch.bfloat16]
want = None
for r in range(2):
    ri, rt = _rank_batch(r, 0)
    torch.manual_seed(5)
    bare.zero_grad()
    sum(bare(ri, rt).values()).backward()
    g = [p.grad.detach().clone() for p in bare.parameters() if p.requires_grad]
    want = g if want is None else [a + b for a, b in zip(want, g)]
want = [w / 2 for w in want]
got = [p.grad for p in m.parameters() if p.requires_grad]
assert len(got) == len(want) > 80
worst = 0.0
for (name, _), a, b in zip([(n, p) for n, p in m.named_parameters() if p.requires_grad], got, want):
    assert a.dtype == torch.float32, name
    err = float((a - b).norm()) / (float(b.norm()) + 1e-12)
    worst = max(worst, err)
    # identical weights and identical (deterministic CPU) operations on both sides, gradients fp32 on both: what differs is the
    # order of the all-reduce's one addition and division -- the fp32 test's step-0 bound
    assert err <= 1e-5, (name, err)
own = [p.grad.detach().clone() for p in bare.parameters() if p.requires_grad]
assert max(float((a - b).norm()) / (float(b.norm()) + 1e-12) for a, b in zip(own, want)) > 1e-2
sys.stdout.write("rank %%d ok worst %%.2e\n" %% (rank, worst))
sys.stdout.flush()
dist.destroy_process_group()
'''


def test_ddp_gloo_gradient_is_the_mean_with_amp(tmp_path):
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    script = tmp_path / "ddp_worker.py"
    script.write_text(_DDP_SCRIPT % ROOT)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), str(script)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "rank 0 ok" in r.stdout and "rank 1 ok" in r.stdout


def test_train_main_then_evaluate_main_with_amp_on_cpu(tmp_path):
    from detectinblur_amd import evaluate, train
    small = ["--synthetic", "--synthetic_images", "6", "--synthetic_size", "96", "128", "--min_size", "96", "--max_size", "128",
             "--device", "cpu", "--amp", "--tensorboard_path", ""]
    ck = tmp_path / "w"
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train.main(train.build_parser().parse_args(small + ["-b", "2", "--epochs", "1", "--lr", "0.001", "--print_freq", "1",
                                                           "--output_dir", str(ck), "--early_stop", "3"]))
    text = buf.getvalue()
    assert "amp=True" in text and "Training time" in text
    losses = [float(x) for x in re.findall(r"loss: ([0-9.eE+-]+|nan|inf)", text)]
    assert len(losses) >= 2 and all(l == l and l < 1e4 for l in losses), text[-1500:]       # three steps (each logged one step later), finite
    state = torch.load(ck / "model_0.pth", map_location="cpu", weights_only=False)
    assert state["args"].amp is True
    assert all(v.dtype == torch.float32 for v in state["model"].values() if v.is_floating_point())
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = evaluate.main(evaluate.build_parser().parse_args(small + ["--vanilla_eval", "--early_stop", "1", "--resume", str(ck / "model_0.pth")]))
    assert len(res["Clean"].coco_eval["bbox"].stats) == 12 and "Loading from" in buf.getvalue()
    # ... and the same checkpoint without the flag
    with contextlib.redirect_stdout(io.StringIO()):
        res = evaluate.main(evaluate.build_parser().parse_args([a for a in small if a != "--amp"] + ["--vanilla_eval", "--early_stop", "1", "--resume",
                                                                                                      str(ck / "model_0.pth")]))
    assert len(res["Clean"].coco_eval["bbox"].stats) == 12


def test_abi_lists_the_bf16_epilogues():
    from detectinblur_amd import _lib
    names = ["dib_bias_act_bf16_nhwc", "dib_bias_act_mask_bf16_nhwc", "dib_relu_mask_backward_bf16", "dib_add_relu_mask_bf16",
             "dib_scatter_add_bf16_nhwc", "dib_fpn_topdown_merge_bf16_nhwc", "dib_stem_pool_forward_bf16", "dib_stem_pool_backward_bf16"]
    l = _lib.lib()
    for n in names:
        assert n in _lib.EXPORTS and getattr(l, n) is not None
    assert l.dib_abi_version() == 7
    # argument errors are reported without a GPU: channel counts that are not a multiple of 8, null pointers
    assert l.dib_bias_act_bf16_nhwc(None, None, None, 48, 12, 1, None) == _lib.DIB_EINVAL and b"C % 8" in l.dib_last_error()
    assert l.dib_bias_act_bf16_nhwc(None, None, None, 64, 16, 1, None) == _lib.DIB_EINVAL and b"null pointer" in l.dib_last_error()
    assert l.dib_add_relu_mask_bf16(None, None, None, 12, None) == _lib.DIB_EINVAL and b"multiple of 8" in l.dib_last_error()
    assert l.dib_scatter_add_bf16_nhwc(16, 16, 1, 4, 4, 3, 3, 8, 2, None) == _lib.DIB_ESHAPE
    # every argument error of both forms of the family: the code, the entry point's own name in front, and the order in which
    # the conditions are tested.  Integers stand in for device pointers (16 = aligned; 17, 24, 40 = not): each row is refused
    # (or found empty) before anything is launched.  dib_bias_act_nhwc has no misalignment row: its answer is the scalar kernel.
    EINVAL, ESHAPE, OK = _lib.DIB_EINVAL, _lib.DIB_ESHAPE, 0
    rows = []
    for sfx, n, bad in (("", 4, 6), ("_bf16", 8, 12)):
        mult = b"n_elems must be a non-negative multiple of %d" % n
        shape = b"_nhwc: bad shape (C %% %d == 0)" % n
        rows += [
            ("dib_relu_mask_backward" + sfx, (None, None, None, bad, None), EINVAL, mult),
            ("dib_relu_mask_backward" + sfx, (16, 16, 16, -n, None), EINVAL, mult),
            ("dib_relu_mask_backward" + sfx, (17, None, None, 0, None), OK, None),
            ("dib_relu_mask_backward" + sfx, (16, None, 16, 2 * n, None), EINVAL, b"dib_relu_mask_backward%s: null pointer" % sfx.encode()),
            ("dib_relu_mask_backward" + sfx, (16, 3, 17, 2 * n, None), EINVAL, b"dib_relu_mask_backward%s: tensors must be 16-byte aligned" % sfx.encode()),
            ("dib_add_relu_mask" + sfx, (None, None, None, bad, None), EINVAL, b"dib_add_relu_mask%s: " % sfx.encode() + mult),
            ("dib_add_relu_mask" + sfx, (None, None, None, 0, None), OK, None),
            ("dib_add_relu_mask" + sfx, (None, 16, None, 2 * n, None), EINVAL, b"dib_add_relu_mask%s: null pointer" % sfx.encode()),
            ("dib_add_relu_mask" + sfx, (16, 24, None, 2 * n, None), EINVAL, b"dib_add_relu_mask%s: tensors must be 16-byte aligned" % sfx.encode()),
            # a, b, N, H, W, Hs, Ws, C, stride: bad shape, then the strided grid (even for N == 0), then N == 0, then the pointers
            ("dib_scatter_add%s_nhwc" % sfx, (16, 16, 1, 4, 4, 2, 2, bad, 2, None), EINVAL, b"dib_scatter_add" + sfx.encode() + shape),
            ("dib_scatter_add%s_nhwc" % sfx, (16, 16, 1, 4, 4, 2, 2, 2 * n, 0, None), EINVAL, b"dib_scatter_add" + sfx.encode() + shape),
            ("dib_scatter_add%s_nhwc" % sfx, (None, None, 0, 4, 4, 3, 3, 2 * n, 2, None), ESHAPE, b"dib_scatter_add%s_nhwc: strided grid leaves the target" % sfx.encode()),
            ("dib_scatter_add%s_nhwc" % sfx, (None, None, 0, 4, 4, 2, 2, 2 * n, 2, None), OK, None),
            ("dib_scatter_add%s_nhwc" % sfx, (None, 16, 1, 4, 4, 2, 2, 2 * n, 2, None), EINVAL, b"dib_scatter_add%s_nhwc: null pointer" % sfx.encode()),
            ("dib_scatter_add%s_nhwc" % sfx, (16, 24, 1, 4, 4, 2, 2, 2 * n, 2, None), EINVAL, b"dib_scatter_add%s_nhwc: tensors must be 16-byte aligned" % sfx.encode()),
            # x, bias, top, N, H, W, Ht, Wt, C
            ("dib_fpn_topdown_merge%s_nhwc" % sfx, (16, 16, 16, 1, 4, 4, 2, 2, bad, None), EINVAL, b"dib_fpn_topdown_merge" + sfx.encode() + shape),
            ("dib_fpn_topdown_merge%s_nhwc" % sfx, (None, None, None, 0, 4, 4, 2, 2, 2 * n, None), OK, None),
            ("dib_fpn_topdown_merge%s_nhwc" % sfx, (16, 16, None, 1, 4, 4, 2, 2, 2 * n, None), EINVAL, b"dib_fpn_topdown_merge%s_nhwc: null pointer" % sfx.encode()),
            ("dib_fpn_topdown_merge%s_nhwc" % sfx, (16, 16, 40, 1, 4, 4, 2, 2, 2 * n, None), EINVAL, b"dib_fpn_topdown_merge%s_nhwc: tensors must be 16-byte aligned" % sfx.encode()),
            # the stem pool takes 4 channels per lane in both forms: x, bias, out, arg, N, H, W, C / grad_out, arg, grad_in, N, H, W, C
            ("dib_stem_pool_forward" + sfx, (16, 16, 16, 16, 1, 8, 8, 6, None), EINVAL, b"dib_stem_pool_forward%s: bad shape (C %% 4 == 0)" % sfx.encode()),
            ("dib_stem_pool_forward" + sfx, (None, None, None, None, 0, 8, 8, 4, None), OK, None),
            ("dib_stem_pool_forward" + sfx, (16, 16, 16, None, 1, 8, 8, 4, None), EINVAL, b"dib_stem_pool_forward%s: null pointer" % sfx.encode()),
            ("dib_stem_pool_forward" + sfx, (16, 16, 24, 16, 1, 131071, 8, 4, None), EINVAL, b"dib_stem_pool_forward%s: tensors must be 16-byte aligned" % sfx.encode()),
            ("dib_stem_pool_forward" + sfx, (16, 16, 16, 16, 1, 131071, 8, 4, None), ESHAPE, b"dib_stem_pool_forward%s: at most 65535 pooled rows and images per call" % sfx.encode()),
            ("dib_stem_pool_forward" + sfx, (16, 16, 16, 16, 65536, 8, 8, 4, None), ESHAPE, b"dib_stem_pool_forward%s: at most 65535 pooled rows" % sfx.encode()),
            ("dib_stem_pool_backward" + sfx, (16, 16, 16, 1, 8, 8, 6, None), EINVAL, b"dib_stem_pool_backward%s: bad shape (C %% 4 == 0)" % sfx.encode()),
            ("dib_stem_pool_backward" + sfx, (None, None, None, 0, 8, 8, 4, None), OK, None),
            ("dib_stem_pool_backward" + sfx, (16, None, 16, 1, 8, 8, 4, None), EINVAL, b"dib_stem_pool_backward%s: null pointer" % sfx.encode()),
            ("dib_stem_pool_backward" + sfx, (24, 16, 16, 1, 65536, 8, 4, None), EINVAL, b"dib_stem_pool_backward%s: tensors must be 16-byte aligned" % sfx.encode()),
            ("dib_stem_pool_backward" + sfx, (16, 16, 16, 1, 65536, 8, 4, None), ESHAPE, b"dib_stem_pool_backward%s: at most 65535 rows and images per call" % sfx.encode()),
            ("dib_stem_pool_backward" + sfx, (16, 16, 16, 65536, 8, 8, 4, None), ESHAPE, b"dib_stem_pool_backward%s: at most 65535 rows" % sfx.encode()),
        ]
    rows += [
        # x, bias, residual, n_elems, C, relu | mask.  The fp32 pair reports the shared checks under dib_bias_act_nhwc's name
        ("dib_bias_act_nhwc", (16, 16, None, 50, 12, 1, None), EINVAL, b"dib_bias_act_nhwc: n_elems must be a multiple of C"),
        ("dib_bias_act_nhwc", (16, 16, None, 48, 0, 1, None), EINVAL, b"dib_bias_act_nhwc: n_elems must be a multiple of C"),
        ("dib_bias_act_nhwc", (None, None, None, 0, 12, 1, None), OK, None),
        ("dib_bias_act_nhwc", (16, None, None, 48, 12, 1, None), EINVAL, b"dib_bias_act_nhwc: null pointer"),
        ("dib_bias_act_mask_nhwc", (16, 16, None, 64, 16, None, None), EINVAL, b"dib_bias_act_mask_nhwc: null mask pointer"),
        ("dib_bias_act_mask_nhwc", (16, 16, None, 60, 6, 16, None), EINVAL, b"dib_bias_act_mask_nhwc: needs C % 4 == 0 and 16-byte aligned tensors"),
        ("dib_bias_act_mask_nhwc", (16, 16, 17, 64, 16, 16, None), EINVAL, b"dib_bias_act_mask_nhwc: needs C % 4 == 0 and 16-byte aligned tensors"),
        ("dib_bias_act_mask_nhwc", (16, 16, None, 50, 16, 16, None), EINVAL, b"dib_bias_act_nhwc: n_elems must be a multiple of C"),
        ("dib_bias_act_mask_nhwc", (None, 16, None, 0, 16, 16, None), OK, None),
        ("dib_bias_act_mask_nhwc", (None, 16, None, 64, 16, 16, None), EINVAL, b"dib_bias_act_nhwc: null pointer"),
        ("dib_bias_act_bf16_nhwc", (16, 16, None, 50, 16, 1, None), EINVAL, b"dib_bias_act_bf16_nhwc: needs C % 8 == 0 and n_elems a multiple of C"),
        ("dib_bias_act_bf16_nhwc", (17, None, None, 0, 16, 1, None), OK, None),
        ("dib_bias_act_bf16_nhwc", (16, 16, 24, 64, 16, 1, None), EINVAL, b"dib_bias_act_bf16_nhwc: tensors must be 16-byte aligned"),
        ("dib_bias_act_mask_bf16_nhwc", (16, 16, None, 48, 12, None, None), EINVAL, b"dib_bias_act_mask_bf16_nhwc: null mask pointer"),
        ("dib_bias_act_mask_bf16_nhwc", (16, 16, None, 48, 12, 16, None), EINVAL, b"dib_bias_act_mask_bf16_nhwc: needs C % 8 == 0"),
        ("dib_bias_act_mask_bf16_nhwc", (16, None, None, 64, 16, 16, None), EINVAL, b"dib_bias_act_mask_bf16_nhwc: null pointer"),
        ("dib_bias_act_mask_bf16_nhwc", (17, 16, None, 64, 16, 16, None), EINVAL, b"dib_bias_act_mask_bf16_nhwc: tensors must be 16-byte aligned"),
    ]
    for name, args, code, text in rows:
        assert getattr(l, name)(*args) == code, (name, args, l.dib_last_error())
        assert text is None or text in l.dib_last_error(), (name, args, l.dib_last_error())


def _device_asm(name):
    """(kernel -> {ScratchSize, Occupancy}, assembly text) of one csrc file compiled for gfx950 with the library's flags."""
    src = os.path.join(ROOT, "detectinblur_amd", "csrc", name)
    asm = os.path.join(os.environ.get("TMPDIR", "/tmp"), "%s_%d.s" % (name, os.getpid()))
    try:
        p = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S", src,
                            "-o", asm, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        text = open(asm).read()
    finally:
        if os.path.exists(asm):
            os.remove(asm)
    out, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    return out, text


def test_bf16_kernels_use_no_scratch():
    """The check of tests/test_mode_one_norm.py::test_mode_one_kernels_use_no_scratch on the epilogue family (the templates of
    csrc/dib_eltwise_vec.h as instantiated for bf16, and for fp32), and that the one rounding per bf16 element is the packed
    hardware conversion."""
    if not os.path.isfile(HIPCC):
        pytest.skip("hipcc not available")
    # kernel stem -> instantiations per lane type (bias_act: residual x ReLU, and the two masked forms; add_mask: with and without)
    family = {"bias_act_kernel": 6, "relu_mask_bwd_kernel": 1, "add_mask_kernel": 2, "scatter_add_kernel": 1,
              "topdown_merge_kernel": 1, "stem_pool_fwd_kernel": 1, "stem_pool_bwd_kernel": 1}
    for name, lane in (("dib_eltwise_bf16.hip", "Bf16Lane"), ("dib_eltwise.hip", "F32Lane")):
        out, text = _device_asm(name)
        other = "F32Lane" if lane == "Bf16Lane" else "Bf16Lane"
        assert not [n for n in out if other in n], name               # the text checks below look at one type's code only
        for frag, count in family.items():
            names = [n for n in out if frag in n and lane in n]
            assert len(names) == count, (frag, names)
            for n in names:
                assert out[n]["ScratchSize"] == 0, (n, out[n])
                assert out[n]["Occupancy"] >= 4, (n, out[n])
        if lane == "Bf16Lane":
            assert len(out) == sum(family.values()), sorted(out)      # nothing but the family in this file
            assert "v_cvt_pk_bf16_f32" in text
            assert "global_load_dwordx4" in text and "global_store_dwordx4" in text        # 16-byte accesses
            assert "global_atomic" not in text and "flat_atomic" not in text
