"""The host references of the trunk's epilogue family (oracle/dib_oracle.py A21: plain numpy float32 / float64, no torch, nothing
of the package) against torch on the CPU, on the random and salted inputs that tests/test_trunk_epilogue_f32_gpu.py feeds to the
HIP kernels: the fp32 additions in the kernels' order, ATen's nearest index (F.interpolate), max_pool2d's values AND indices --
windows with one and with several NaN included: the LAST NaN in row-major window order is ATen's index --, and the ReLU, which
equals torch's everywhere except the sign of a zero result (torch.relu(-0.0) is -0.0 on the CPU; the kernels, and the "cleared
elements are +0" rule of the mask kernels, give +0.0).  Also the one place where the mask form and torch part ways on purpose:
a NaN output carries no mask bit, where threshold_backward(g, NaN, 0) passes g.

This module also builds the inputs (numpy, channels-last) that both halves use."""
import numpy as np
import torch

import dib_oracle as O
from tests.test_amp_gpu import SPECIALS

F = torch.nn.functional
INF, NAN = float("inf"), float("nan")

# (N, C, H, W): ragged toy shapes (more than one block, no multiple of anything), one pixel, and one mid-size trunk level
SHAPES = [(3, 8, 5, 7), (2, 64, 37, 53), (1, 4, 1, 1), (1, 256, 50, 84)]
SCALAR_SHAPE = (2, 6, 5, 7)                       # C % 4 != 0: the scalar kernel
TRANSPOSE_SHAPES = [(1, 4, 3, 5), (3, 68, 7, 9)]
SCATTER_CASES = [(2, 64, 37, 53, 2), (3, 8, 5, 7, 2), (1, 16, 8, 6, 2), (2, 16, 9, 6, 3)]          # (N, C, H, W, stride): odd and even sizes
TOPDOWN_CASES = [(8, 256, 50, 84, 25, 42), (2, 256, 51, 101, 26, 51), (1, 64, 7, 9, 4, 5), (3, 8, 33, 20, 11, 7)]
STEM_SHAPES = [(2, 64, 40, 56), (1, 64, 37, 51), (3, 8, 9, 12), (1, 4, 1, 1), (1, 4, 2, 5)]


def rand_nhwc(shape, seed, specials=True, roll=0):
    """[N, H, W, C] float32: random values, and the special values spread over channels 0..3 of a few pixels (the layout of
    tests/test_amp_gpu._rand: special k at pixel 3 k + seed % 5).  `roll` rotates the list, so that two tensors with equal
    seed % 5 meet as (inf, -inf), (-inf, NaN), ... under an addition."""
    N, C, H, W = shape
    rs = np.random.RandomState(seed)
    t = rs.standard_normal((N, H, W, C)).astype(np.float32)
    if specials:
        flat = t.reshape(-1)
        vals = np.roll(np.array(SPECIALS, dtype=np.float32), -roll)
        for c in range(min(4, C)):
            idx = (np.arange(len(vals)) * 3 + seed % 5) * C + c
            idx = idx[idx < flat.size]
            flat[idx] = vals[:len(idx)]
    return t


def rand_bias(C, seed):
    """0.0, -0.0 and fp32's smallest denormal on channels 0..2 (x = 0 plus that is a positive sum), random elsewhere"""
    b = np.random.RandomState(1000 + seed).standard_normal(C).astype(np.float32)
    b[0] = 0.0
    if C > 1:
        b[1] = -0.0
    if C > 2:
        b[2] = 1e-45
    return b


def stem_input(shape, seed):
    """the existing stem test's input (exact ties between neighbours, positive and negative) plus +-inf and NaN pixels placed so
    that a NaN is alone in a window, shared by two and by four overlapping windows, on a border, and together with a second NaN
    (two different payload-free positions) in one window.  Returns x [N, H, W, C], bias [C]."""
    N, C, H, W = shape
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((N, H, W, C)).astype(np.float32)
    if H > 2 and W > 2:
        dst = x[:, 1::3, 1::4]
        dst[...] = x[:, 0::3, 0::4][:, :dst.shape[1], :dst.shape[2]]
    bias = rs.standard_normal(C).astype(np.float32)
    bias[0] = 0.0
    if H >= 9 and W >= 12:
        n = N - 1
        x[n, 2, 2, :] = NAN          # even row, even column: ONE window (1, 1)
        x[n, 2, 7, :] = NAN          # even row, odd column: two windows
        x[n, 5, 9, :] = NAN          # odd row, odd column: four windows
        x[n, 0, 5, :] = NAN          # top border
        x[n, H - 1, 0, :] = NAN      # bottom-left corner
        x[n, 7, 3, 0::2] = NAN       # two NaN in the windows around (7, 3) / (8, 4), on every other channel
        x[n, 8, 4, 0::2] = NAN
        x[0, 4, 4, :] = INF
        x[0, 6, 10, :] = -INF
        x[0, 6, 11, 1::2] = NAN      # a NaN next to -inf
    elif H * W > 1:
        x[0, H - 1, W - 1, 1] = NAN  # the 2 x 5 case: a corner
        x[0, 0, 2, 2] = INF
    return x, bias


def nchw(t):
    return torch.from_numpy(np.ascontiguousarray(t)).permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def same_bits(got, want):
    """bit for bit; NaN by position, not by payload"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    kind = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(np.where(gn, 0, got.view(kind)), np.where(wn, 0, want.view(kind))))


def same_up_to_the_sign_of_zero(ref, tor):
    """NaN at equal positions, equal values (so -0.0 == +0.0), and the reference's zeros are all +0.0"""
    rn, tn = np.isnan(ref), np.isnan(tor)
    ok = np.array_equal(rn, tn) and np.array_equal(np.where(rn, 0, ref), np.where(tn, 0, tor))
    return bool(ok and not np.signbit(ref[ref == 0]).any() and same_bits(np.where(tor == 0, np.float32(0), tor), ref))


def test_relu_reference_is_torchs_up_to_the_sign_of_a_zero_result():
    v = np.array(SPECIALS + [-1.0, 2.5, -1e-45, 1e-45], dtype=np.float32)
    r, t = O.relu32(v), torch.relu(torch.from_numpy(v)).numpy()
    assert same_up_to_the_sign_of_zero(r, t)
    assert np.isnan(r[2]) and r[0] == INF and r[1] == 0 and r[-1] == np.float32(1e-45)
    assert np.signbit(t[4]) and not np.signbit(r[4])             # the one difference: relu(-0.0)


def test_bias_act_reference_equals_the_torch_expression():
    hit_nan = False
    for k, shape in enumerate(SHAPES + [SCALAR_SHAPE]):
        C = shape[1]
        x, r, bias = rand_nhwc(shape, 10 + k), rand_nhwc(shape, 50 + k, roll=1), rand_bias(C, k)
        for res in (None, r):
            v = nchw(x) + torch.from_numpy(bias).reshape(1, -1, 1, 1)
            if res is not None:
                v = v + nchw(res)
            assert same_bits(O.bias_act32(x, bias, res, False), nhwc(v)), (shape, res is not None)
            got = O.bias_act32(x, bias, res, True)
            assert same_up_to_the_sign_of_zero(got, nhwc(torch.relu(v))), (shape, res is not None)
            if res is not None:
                hit_nan |= bool((np.isnan(got) & ~np.isnan(x) & ~np.isnan(r)).any())       # inf - inf: a NaN born in the kernel
            # the mask against threshold_backward: equal wherever the output is not NaN; a NaN output passes g in torch and
            # carries no bit here
            g = np.random.RandomState(k).standard_normal(got.shape).astype(np.float32)
            mine = O.mask_select(g, O.sign_mask(got))
            tor = nhwc(torch.ops.aten.threshold_backward(nchw(g), nchw(got), 0)) if C % 4 == 0 else None
            if tor is not None:
                nan = np.isnan(got)
                assert np.array_equal(mine[~nan], tor[~nan]) and not mine[nan].any() and np.array_equal(tor[nan], g[nan])
                assert not np.signbit(mine[mine == 0]).any()
    assert hit_nan


def test_mask_round_trip_and_add_relu_mask_reference():
    for k, shape in enumerate(SHAPES):
        a, b = rand_nhwc(shape, 20 + k), rand_nhwc(shape, 30 + k, roll=1)
        mask = np.random.RandomState(k).randint(0, 16, a.size // 4).astype(np.uint8)
        keep = O.mask_bits(mask).reshape(a.shape)
        assert np.array_equal(O.sign_mask(np.where(keep, np.float32(1), np.float32(-1))), mask)
        s = nhwc(nchw(a) + nchw(b))
        assert same_bits(O.add_relu_mask32(a, b), s)
        want = np.where(keep, s, np.float32(0))
        got = O.add_relu_mask32(a, b, mask)
        assert same_bits(got, want) and not got[~keep].view(np.uint32).any()


def test_scatter_add_reference_equals_strided_assignment():
    for k, (N, C, H, W, s) in enumerate(SCATTER_CASES):
        Hs, Ws = (H - 1) // s + 1, (W - 1) // s + 1
        a, b = rand_nhwc((N, C, H, W), 40 + k), rand_nhwc((N, C, Hs, Ws), 60 + k, roll=1)
        want = nchw(a).clone()
        want[:, :, ::s, ::s] = want[:, :, ::s, ::s] + nchw(b)
        assert same_bits(O.scatter_add32(a, b, s), nhwc(want))


def test_topdown_reference_equals_interpolate_nearest():
    for k, (N, C, H, W, Ht, Wt) in enumerate(TOPDOWN_CASES):
        x, top, bias = rand_nhwc((N, C, H, W), 70 + k), rand_nhwc((N, C, Ht, Wt), 80 + k, roll=1), rand_bias(C, 7 + k)
        want = (nchw(x) + torch.from_numpy(bias).reshape(1, -1, 1, 1)) + F.interpolate(nchw(top), size=(H, W), mode="nearest")
        assert same_bits(O.topdown_merge32(x, bias, top), nhwc(want)), (N, C, H, W)
    for out, inn in ((50, 25), (51, 26), (101, 51), (7, 4), (33, 11), (20, 7), (9, 5), (1333, 667), (5, 5), (3, 1)):
        ramp = torch.arange(inn, dtype=torch.float32).reshape(1, 1, inn, 1)
        assert np.array_equal(O.nearest_src(out, inn), F.interpolate(ramp, size=(out, 1), mode="nearest").reshape(-1).long().numpy()), (out, inn)


def _torch_index_of(pos, H, W):
    """window position 0..8 of pooled element (oh, ow) -> ATen's flat index h * W + w into the input plane"""
    N, Ho, Wo, C = pos.shape
    oh, ow = np.arange(Ho).reshape(1, -1, 1, 1), np.arange(Wo).reshape(1, 1, -1, 1)
    p = pos.astype(np.int64)
    return (oh * 2 - 1 + p // 3) * W + (ow * 2 - 1 + p % 3)


def test_stem_pool_reference_equals_max_pool2d_values_and_indices_nan_windows_included():
    windows_with_two_nan = 0
    for k, shape in enumerate(STEM_SHAPES):
        N, C, H, W = shape
        x, bias = stem_input(shape, k)
        pooled, pos = O.stem_pool32(x, bias)
        act = torch.relu(nchw(x) + torch.from_numpy(bias).reshape(1, -1, 1, 1))
        want, idx = F.max_pool2d(act, 3, stride=2, padding=1, return_indices=True)
        assert same_up_to_the_sign_of_zero(pooled, nhwc(want)), shape
        live = pos != 15
        assert np.array_equal(_torch_index_of(pos, H, W)[live], nhwc(idx)[live]), shape            # NaN windows are live
        assert np.array_equal(live, np.isnan(pooled) | (pooled > 0)) and (nhwc(want)[~live] == 0).all()
        if H >= 9 and W >= 12:
            assert np.isnan(pooled).any() and (pooled == INF).any()
            # the last NaN of a window wins: the window (4, 2) holds (7, 3) and (8, 4); position of (8, 4) there is 1 * 3 + 1 = 4
            assert np.isnan(pooled[N - 1, 4, 2, 0]) and pos[N - 1, 4, 2, 0] == 4 and pos[N - 1, 4, 2, 1] != 4
            a = nhwc(act)
            nan_count = sum(np.isnan(np.pad(a[N - 1], ((1, 2), (1, 2), (0, 0)), constant_values=0)[i // 3:i // 3 + 2 * pos.shape[1]:2,
                                                                                                  i % 3:i % 3 + 2 * pos.shape[2]:2]).astype(int) for i in range(9))
            windows_with_two_nan += int((nan_count >= 2).sum())
        # the rule without the ReLU's zero plateau: shifted up, every window has a positive maximum and every index compares
        up = x + np.float32(10.0)
        pooled, pos = O.stem_pool32(up, np.zeros(C, np.float32))
        want, idx = F.max_pool2d(nchw(up), 3, stride=2, padding=1, return_indices=True)
        assert (pos != 15).all() and same_bits(pooled, nhwc(want)) and np.array_equal(_torch_index_of(pos, H, W), nhwc(idx)), shape
        # backward: autograd through relu and max_pool2d in float64 (threshold_backward passes the gradient at a NaN)
        xa = (nchw(x).double() + torch.from_numpy(bias).double().reshape(1, -1, 1, 1)).requires_grad_(True)
        y = F.max_pool2d(torch.relu(xa), 3, stride=2, padding=1)
        g = torch.from_numpy(np.random.RandomState(k).standard_normal(y.shape))
        y.backward(g)
        _, pos = O.stem_pool32(x, bias)
        mine = O.stem_pool_backward64(nhwc(g), pos, H, W)
        assert np.allclose(mine, nhwc(xa.grad), rtol=1e-12, atol=1e-12), shape
    assert windows_with_two_nan > 0


def test_bf16_rounding_reference_equals_torchs_cast():
    v = np.concatenate([np.array(SPECIALS, dtype=np.float32), rand_nhwc((1, 8, 9, 11), 3).reshape(-1),
                        np.array([1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 3.4e38, -3.4e38, 1e-45], dtype=np.float32)])
    mine = O.from_bf16_bits(O.to_bf16_bits(v))
    tor = torch.from_numpy(v).to(torch.bfloat16).float().numpy()
    assert same_bits(mine, tor)
