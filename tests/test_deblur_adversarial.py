"""`train_deblurrer.py --loss ...+w*ADV` without a GPU: the discriminator against the reference's own module (a recorded fixture), the
193 rule, the --loss grammar and its refusals, the torch restatements of the LeakyReLU and loss kernels against torch and float64, the
D update alone, and the driver on the CPU: checkpoint layout, the default left as it was, --resume, two ranks over gloo.

`python tests/test_deblur_adversarial.py --write` rewrites tests/golden/discriminator_pins.npz from the live reference's
models/deblur/discriminator.py on CPU (DIB_REFERENCE_ROOT, default /root/reference): a seeded state dict at n_feats 4 (every layer
scaled up so that the logits are of magnitude 0.1 to 10; the default initialisation gives 1e-3) and the logits of a 196 x 196 batch of
two and of one 449 x 196 image (a 2 x 1 map).  The inputs are the closed-form integer pattern `pattern` below and are not stored.
Data only."""
import contextlib
import io
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "discriminator_pins.npz")
TINY = ["--n_scales", "2", "--n_resblocks", "2", "--n_feats", "8", "--kernel_size", "5"]      # tests/test_deblur_train.py's
LAYER_SCALE = 1.45
SPECIALS = [-100.0, -20.0, -1e-8, -0.0, 0.0, 1e-8, 0.3, 20.0, 100.0]


def pattern(B, H, W):
    """[B, 3, H, W] of integers 0..255, closed form"""
    b, c, i, j = torch.meshgrid(torch.arange(B), torch.arange(3), torch.arange(H), torch.arange(W), indexing="ij")
    return ((i * 7 + j * 13 + c * 29 + b * 51 + (i * j) % 17 * 5) % 256).float()


def write_fixture():
    import types
    sys.path.insert(0, os.environ.get("DIB_REFERENCE_ROOT", "/root/reference"))
    from models.deblur.discriminator import Discriminator as Reference
    torch.manual_seed(20261020)
    net = Reference(types.SimpleNamespace(n_feats=4, kernel_size=5)).eval()
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(LAYER_SCALE)
        out_a, out_b = net(pattern(2, 196, 196)), net(pattern(1, 449, 196))
    data = {"sd/" + k: v.numpy() for k, v in net.state_dict().items()}
    data.update({"logits_196": out_a.numpy(), "logits_449x196": out_b.numpy()})
    np.savez_compressed(FIXTURE, **data)
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes,", len(data), "arrays; logits", out_a.flatten().tolist(), out_b.flatten().tolist())


@pytest.fixture(scope="module")
def pins():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def fixture_state(pins):
    return {k[3:]: torch.from_numpy(v.copy()) for k, v in pins.items() if k.startswith("sd/")}


KEYS = ["conv_layers.%d.weight" % i for i in range(10)] + ["dense.weight"]


# ---- the network -----------------------------------------------------------------------------------------------------------------

def test_state_dict_and_logits_are_the_references(pins):
    from detectinblur_amd.models.deblur_adversarial import Discriminator, discriminator_forward
    state = fixture_state(pins)
    net = Discriminator(n_feats=4, kernel_size=5)
    own = net.state_dict()
    assert list(own) == list(state) == KEYS and all(own[k].shape == state[k].shape for k in state)
    assert sum(v.numel() for v in state.values()) == 42066 and os.path.getsize(FIXTURE) < 250_000
    net.load_state_dict(state, strict=True)
    with torch.no_grad():
        a, b = discriminator_forward(net, pattern(2, 196, 196)), discriminator_forward(net, pattern(1, 449, 196))
    assert net.last_path == "torch" and a.shape == (2, 1, 1, 1) and b.shape == (1, 1, 2, 1)
    for got, key in ((a, "logits_196"), (b, "logits_449x196")):
        err = float(np.abs(got.numpy() - pins[key]).max())
        print(key, pins[key].flatten().tolist(), "max abs error", err)
        assert (np.abs(pins[key]) >= 0.1).all() and (np.abs(pins[key]) <= 10).all()      # the recorded logits say something
        assert err <= 1e-4                                                              # tests/test_deblur_first.py's rule
    big = Discriminator()                                                               # the defaults are DeepDeblur's
    sd = big.state_dict()
    assert [tuple(sd[k].shape) for k in KEYS] == [(32, 3, 5, 5), (32, 32, 5, 5), (64, 32, 5, 5), (64, 64, 5, 5), (128, 64, 5, 5), (128, 128, 5, 5),
                                                  (256, 128, 5, 5), (256, 256, 5, 5), (512, 256, 5, 5), (512, 512, 4, 4), (1, 512, 1, 1)]
    assert [c.stride[0] for c in big.conv_layers] == [1, 2, 1, 2, 1, 4, 1, 4, 1, 4] and big.conv_layers[9].padding == (0, 0)


def test_the_smaller_side_must_be_at_least_193():
    from detectinblur_amd.models import deblur_adversarial as DA
    net = DA.Discriminator(n_feats=4)
    assert DA.min_side(5) == 193 and DA.final_side(192) == 0 and [DA.final_side(n) for n in (193, 196, 256, 449)] == [1, 1, 1, 2]
    with torch.no_grad():
        with pytest.raises(ValueError, match="193"):
            DA.discriminator_forward(net, torch.zeros(1, 3, 192, 200))
        with pytest.raises(ValueError, match="193"):
            net(torch.zeros(1, 3, 200, 192))
        assert DA.discriminator_forward(net, torch.zeros(2, 3, 193, 200)).shape == (2, 1, 1, 1)
    assert net.activation_shapes(2, 196, 196) == [(2, 2, 196, 196), (2, 2, 98, 98), (2, 4, 98, 98), (2, 4, 49, 49), (2, 8, 49, 49),
                                                  (2, 8, 13, 13), (2, 16, 13, 13), (2, 16, 4, 4), (2, 32, 4, 4), (2, 32, 1, 1)]


# ---- --loss ------------------------------------------------------------------------------------------------------------------------

def test_loss_grammar_and_refusals():
    from detectinblur_amd import train_deblurrer as TD
    assert TD.parse_loss("1*L1") == {"L1": 1.0} and TD.build_parser().parse_args([]).loss == "1*L1"
    assert TD.parse_loss("1*L1+3*ADV") == {"L1": 1.0, "ADV": 3.0}
    assert TD.parse_loss("0.5*adv+1*l1") == {"ADV": 0.5, "L1": 1.0}
    for spec, message in (("1*L1+1*MSE", "'MSE' is not built"), ("1*L1+2*l1", "L1 is given twice"), ("1*L1+ADV", "'ADV' has no weight"),
                          ("*L1", "'\\*L1' has no weight"), ("inf*L1", "weight 'inf' of the term 'inf\\*L1' needs to be finite and above 0"),
                          ("1*L1+0*ADV", "weight '0' of the term '0\\*ADV'"), ("-1*ADV", "weight '-1'"), ("nan*L1", "weight 'nan'"),
                          ("x*L1", "weight 'x' of the term 'x\\*L1' is not a number"), ("", "needs at least one of L1 and ADV")):
        with pytest.raises(SystemExit, match=message):
            TD.parse_loss(spec)
        with pytest.raises(SystemExit, match=message):
            TD.main(["--synthetic", "--device", "cpu", "--loss=" + spec])      # (= form: -1*ADV begins like a flag)
    with pytest.raises(SystemExit, match="--patch_size 192.*at least 193"):
        TD.main(["--synthetic", "--device", "cpu", "--loss", "1*L1+1*ADV", "--patch_size", "192"])


# ---- the restatements ------------------------------------------------------------------------------------------------------------

def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_leaky_restatements_are_torchs_bit_for_bit(dtype):
    from detectinblur_amd.models import deblur_adversarial as DA
    from detectinblur_amd.models.deblur_train import sign_mask_torch
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(4099 * 8, generator=g) * torch.rand(4099 * 8, generator=g).mul(8).sub(6).exp()).to(dtype)
    x[:6] = torch.tensor([0.0, -0.0, 65504.0, -65504.0, 6e-8, -6e-8]).to(dtype)          # zeros, Half's largest, Half denormals
    y, mask = DA.leaky_mask_torch(x)
    leaf = x.clone().requires_grad_(True)
    want = F.leaky_relu(leaf, 0.2)
    assert torch.equal(_bits(y), _bits(want.detach())) and y[1] == 0 and torch.signbit(y[1])
    assert torch.equal(mask, sign_mask_torch(y)) and mask.numel() == x.numel() // (8 if dtype == torch.float16 else 4)
    assert torch.equal(mask, sign_mask_torch(x))                                       # slope > 0: the mask of the result is the input's
    grad = torch.randn(x.shape, generator=g).to(dtype)
    want.backward(grad)
    assert torch.equal(_bits(DA.leaky_grad_torch(grad, mask)), _bits(leaf.grad))
    nan = DA.leaky_mask_torch(torch.full((8,), float("nan"), dtype=dtype))
    assert torch.isnan(nan[0]).all() and int(nan[1].sum()) == 0


def bce_float64(x, label):
    """the float64 statement of csrc/dib_deblur_adv.hip's formulas -> (per-element gradient without the 1 / n, per-element term)"""
    z = -x.double() if label else x.double()
    e = torch.exp(-z.abs())
    sigma = torch.where(z >= 0, 1 / (1 + e), e / (1 + e))
    return (-sigma if label else sigma), z.clamp_min(0) + torch.log1p(e)


@pytest.mark.parametrize("label", [0, 1])
def test_adv_bce_restatement_against_float64_and_torch(label):
    from detectinblur_amd.models import deblur_adversarial as DA
    x = torch.tensor(SPECIALS + (torch.randn(40, generator=torch.Generator().manual_seed(5)) * 8).tolist())
    n = x.numel()
    grad, term = DA.adv_bce_terms_torch(x, label, gscale=0.5)
    g64, t64 = bce_float64(x, label)
    want = float(t64.sum() / n)
    assert abs(float(term) - want) <= (n + 4) * 2.0 ** -24 * want
    tiny = float(np.finfo(np.float32).tiny)
    rel = ((grad.double() - 0.5 * g64 / n).abs() / (0.5 * g64 / n).abs().clamp_min(tiny)).max()
    print("label", label, "loss", float(term), want, "worst relative gradient error", float(rel))
    assert rel <= 8 * 2.0 ** -24
    half_k = float(np.float32(0.5) / np.float32(n) * np.float32(0.5))
    assert abs(float(grad[4])) == half_k and abs(float(grad[3])) == half_k                # sigma(+-0) = 1 / 2
    # the node: value and gradient against torch's own
    leaf = x.clone().requires_grad_(True)
    loss = DA.adv_bce(leaf, label)
    (3.0 * loss).backward()
    other = x.clone().requires_grad_(True)
    ref = F.binary_cross_entropy_with_logits(other, torch.full_like(x, float(label)))
    (3.0 * ref).backward()
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-6 * float(ref.detach())
    # torch's gradient is sigmoid(x) - label: next to 1 its sigmoid is good to a few units of 2^-24, and that is all the difference keeps
    assert torch.allclose(leaf.grad, other.grad, rtol=1e-6, atol=3.0 * 4 * 2.0 ** -24 / n)
    # a NaN logit: its own gradient element and the loss, nothing else; +-inf follows the formulas
    bad = x.clone()
    bad[7] = float("nan")
    g, t = DA.adv_bce_terms_torch(bad, label)
    assert torch.isnan(t) and torch.isnan(g[7]) and int(torch.isnan(g).sum()) == 1
    g, t = DA.adv_bce_terms_torch(torch.tensor([float("inf"), float("-inf")]), label)
    assert g.tolist() == ([0.0, -0.5] if label else [0.5, 0.0]) and float(t) == float("inf")
    assert DA.adv_loss_depth(1) == 1 + 8 + 0 and DA.adv_loss_depth(2049) == 5 + 8 + 1 and DA.adv_loss_depth(2048 * 1024 + 5) == 9 + 8 + 1023
    both = DA.adv_bce_sum([(x, 0), (x[:5], 1)])
    assert abs(float(both) - float(DA.adv_bce(x, 0)) - float(DA.adv_bce(x[:5], 1))) <= 1e-6
    with pytest.raises(ValueError):
        DA.adv_bce(x, 2)


def test_discriminator_learns_to_tell_two_fixed_batches_apart():
    from detectinblur_amd.models import deblur_adversarial as DA
    torch.manual_seed(8)
    D = DA.Discriminator(n_feats=8)
    real = pattern(2, 196, 196)
    fake = (real + torch.roll(real, 1, 3) + torch.roll(real, 1, 2)) / 3
    opt = torch.optim.Adam(D.parameters(), lr=1e-4)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = DA.discriminator_loss(lambda x: DA.discriminator_forward(D, x), fake, real)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("loss_d", losses[0], "->", losses[-1])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] and abs(losses[0] - 2 * np.log(2)) < 0.1


# ---- the driver ------------------------------------------------------------------------------------------------------------------

ADV = ["--loss", "1*L1+1*ADV"]


def _run(out_dir, *extra):
    from detectinblur_amd import train_deblurrer as TD
    argv = ["--synthetic", "--synthetic_images", "4", "--synthetic_size", "200", "216", "--device", "cpu", "-j", "0", "-b", "2",
            "--patch_size", "196", "--print_freq", "1", "--output_dir", str(out_dir)] + TINY + list(extra)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        TD.main(argv)
    return buf.getvalue()


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """two epochs (of two steps) with ADV, saved after each; one epoch of the default; one epoch of an explicit --loss 1*L1"""
    d = tmp_path_factory.mktemp("adv")
    text = _run(d / "adv", "--epochs", "2", "--save_every", "1", *ADV)
    _run(d / "default", "--epochs", "1")
    _run(d / "l1", "--epochs", "1", "--loss", "1*L1")
    return d, text


def test_driver_with_adv_on_the_cpu(runs, pins):
    import re
    from detectinblur_amd.models import deblur
    d, text = runs
    rows = re.findall(r"loss: (\S+)  lr: \S+  path: torch  adv: (\S+)  d: (\S+)  d_path: torch\n", text)
    assert len(rows) == 4 and all(np.isfinite(float(v)) for row in rows for v in row), text[-2000:]
    model = _load(d / "adv" / "models" / "model-1.pt")
    assert set(model) == {"G", "D"} and list(model["D"]) == KEYS == list(fixture_state(pins))
    assert model["D"]["conv_layers.0.weight"].shape == (4, 3, 5, 5)                 # the generator's n_feats, as in the reference
    with contextlib.redirect_stdout(io.StringIO()):
        deblurer = deblur.Deblurer(str(d / "adv"))                                  # reads "G", ignores the rest
    out = deblurer.deblur_(torch.rand(3, 20, 28))
    assert out.shape == (3, 20, 28) and torch.isfinite(out).all()
    optim = torch.load(d / "adv" / "optim" / "optim-1.pt", map_location="cpu", weights_only=False)
    assert {"optimizer", "optimizer_D", "lr_scheduler", "lr_scheduler_D"} <= set(optim) and optim["args"]["loss"] == "1*L1+1*ADV"
    assert len(optim["optimizer_D"]["state"]) == 11
    plain = _load(d / "default" / "models" / "model-1.pt")
    assert any(not torch.equal(model["G"][k], plain["G"][k]) for k in plain["G"])   # the adversarial term reaches the generator


class _Recorder(object):
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, tag, value, step):
        self.scalars.setdefault(tag, []).append(value)

    def flush(self):
        pass

    close = flush


@pytest.mark.parametrize("spec,tags", [("2*ADV", {"losses/adv_g", "losses/adv_d"}), ("3*L1", {"losses/l1_pyramid"}),
                                       ("3*L1+2*ADV", {"losses/l1_pyramid", "losses/adv_g", "losses/adv_d"})])
def test_tensorboard_tags_hold_the_unweighted_terms(tmp_path, monkeypatch, spec, tags):
    """`loss:` is the weighted total; losses/l1_pyramid is the L1 term itself and is written only when --loss has one"""
    import re
    from detectinblur_amd import tb_writer
    rec = _Recorder()
    monkeypatch.setattr(tb_writer, "make_writer", lambda path: rec)
    text = _run(tmp_path, "--epochs", "1", "--early_stop", "0", "--tensorboard_path", str(tmp_path / "tb"), "--loss", spec)
    assert {t for t in rec.scalars if t.startswith("losses/")} == tags
    total = float(re.search(r"loss: (\S+)", text).group(1))
    l1 = rec.scalars.get("losses/l1_pyramid", [0.0])[0]
    adv = rec.scalars.get("losses/adv_g", [0.0])[0]
    assert 80 < l1 < 90 or "L1" not in spec                     # the unweighted term of these synthetic pairs, whatever its weight
    assert abs(total - ((3 * l1 if "L1" in spec else 0) + (2 * adv if "ADV" in spec else 0))) <= 1e-3 * total + 1e-4


def test_an_explicit_l1_is_the_default_run_bit_for_bit(runs):
    d, _ = runs
    a, b = _load(d / "default" / "models" / "model-1.pt"), _load(d / "l1" / "models" / "model-1.pt")
    assert set(a) == set(b) == {"G"} and all(torch.equal(a["G"][k], b["G"][k]) for k in a["G"])
    optim = torch.load(d / "l1" / "optim" / "optim-1.pt", map_location="cpu", weights_only=False)
    assert "optimizer_D" not in optim and "lr_scheduler_D" not in optim


def test_resume_restores_generator_and_discriminator_bit_for_bit(runs, tmp_path):
    d, _ = runs
    _run(tmp_path, "--epochs", "1", "--save_every", "1", *ADV)
    text = _run(tmp_path, "--epochs", "2", "--save_every", "1", "--resume", *ADV)
    assert "Resumed from" in text and "Epoch: [2]" in text and "Epoch: [1]" not in text
    a, b = _load(d / "adv" / "models" / "model-2.pt"), _load(tmp_path / "models" / "model-2.pt")
    first = _load(d / "adv" / "models" / "model-1.pt")
    for part in ("G", "D"):
        assert set(a[part]) == set(b[part]) and all(torch.equal(a[part][k], b[part][k]) for k in a[part]), part
        assert any(not torch.equal(a[part][k], first[part][k]) for k in a[part]), part      # the second epoch did train
    with pytest.raises(SystemExit, match=r"was written with --loss 1\*L1\+1\*ADV and this run is with --loss 1\*L1"):
        _run(tmp_path, "--epochs", "2", "--resume")
    with pytest.raises(SystemExit, match=r"was written with --loss 1\*L1 and this run is with --loss 2\*ADV"):
        _run(d / "default", "--epochs", "2", "--resume", "--loss", "2*ADV")


# ---- two ranks over gloo (tests/test_drivers_two_ranks.py's way) --------------------------------------------------------------------

_WORKER = r'''
import os, sys
sys.path.insert(0, %(root)r)
import torch
from detectinblur_amd import train_deblurrer
outdir, argv = sys.argv[1], sys.argv[2:]
trainer = train_deblurrer.main(argv)
torch.save({"G": trainer.bare.state_dict(), "D": trainer.bare_d.state_dict()}, os.path.join(outdir, "rank%%s.pt" %% os.environ.get("RANK", "0")))
'''


def test_two_ranks_over_gloo_keep_generator_and_discriminator_in_step(tmp_path):
    from detectinblur_amd import train_deblurrer as TD
    worker = tmp_path / "worker.py"
    worker.write_text(_WORKER % {"root": ROOT})
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, OMP_NUM_THREADS="2", MASTER_ADDR="127.0.0.1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    flags = ["--synthetic", "--synthetic_images", "8", "--synthetic_size", "200", "216", "--device", "cpu", "-j", "0", "-b", "2", "--patch_size", "196",
             "--print_freq", "1", "--epochs", "1", "--early_stop", "1", "--output_dir", str(tmp_path / "out")] + TINY + ADV
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           str(worker), str(tmp_path)] + flags
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "d_path: torch" in r.stdout
    ranks = [_load(tmp_path / ("rank%d.pt" % k)) for k in range(2)]
    args = TD.build_parser().parse_args(flags)
    args.distributed = False
    fresh = TD.Trainer(args, torch.device("cpu"))
    initial = {"G": fresh.bare.state_dict(), "D": fresh.bare_d.state_dict()}
    for part in ("G", "D"):
        a, b = ranks[0][part], ranks[1][part]
        assert set(a) == set(b) == set(initial[part])
        assert all(torch.equal(a[k], b[k]) for k in a), part
        assert any(not torch.equal(a[k], initial[part][k]) for k in a), part
    saved = _load(tmp_path / "out" / "models" / "model-1.pt")
    assert set(saved) == {"G", "D"} and all(torch.equal(saved["D"][k], ranks[0]["D"][k]) for k in saved["D"])


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        write_fixture()
    else:
        sys.exit("usage: python tests/test_deblur_adversarial.py --write")
