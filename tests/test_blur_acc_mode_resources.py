"""Register, scratch and occupancy budget of the fused blur + normalise kernels that `--blur_acc_mode fp32 / fast16` added
(blur_quad_f16_norm_kernel<DIB_ACC_FAST16, 128>, <DIB_ACC_FP32, 128>, <DIB_ACC_FP32, 256>), read from hipcc's own resource report of
csrc/dib_blur.hip -- the pattern of tests/test_kernel_resources.py, whose reasons apply: no scratch, and no fewer waves per SIMD than
the kernel that runs the same mode WITHOUT the normalising store.  Those siblings stood at 8 waves per SIMD before the fused forms
existed (blur_quad_f16_kernel<FAST16, 128>: 64 VGPRs / 74 SGPRs; blur_quad_f32acc_kernel<128>: 59 / 76; <256>: 51 / 68), so 8 it is,
which on gfx950 means <= 64 vector registers per lane and <= 80 scalar registers per wave.  A fused form that cannot hold this is
to be left out of dib_sparse_blur_normalized (the caller then takes two launches), never shipped spilling."""
import pytest

from tests.test_kernel_resources import report  # noqa: F401  (the module-scoped fixture: one hipcc run for this file)

# mangled-name fragment of the fused kernel -> (fragment of its non-NORM sibling, waves per SIMD of that sibling)
FUSED = {
    "blur_quad_f16_norm_kernelILi3ELi128E": ("blur_quad_f16_kernelILi3ELi128ELb0E", 8),   # FAST16
    "blur_quad_f16_norm_kernelILi1ELi128E": ("blur_quad_f32acc_kernelILi128E", 8),        # FP32
    "blur_quad_f16_norm_kernelILi1ELi256E": ("blur_quad_f32acc_kernelILi256E", 8),
}


def _one(report, fragment):  # noqa: F811
    names = [n for n in report if fragment in n]
    assert len(names) == 1, (fragment, names)
    return report[names[0]]


@pytest.mark.parametrize("kernel", list(FUSED))
def test_fused_tolerance_mode_kernels_hold_their_siblings_budget(report, kernel):  # noqa: F811
    sibling, waves = FUSED[kernel]
    r, s = _one(report, kernel), _one(report, sibling)
    assert r["ScratchSize"] == 0, r
    assert r["Occupancy"] >= waves and r["Occupancy"] >= s["Occupancy"], (r, s)
    assert r["VGPRs"] <= 64 and r["TotalSGPRs"] <= 80, r


def test_the_fused_forms_that_existed_before_are_still_there(report):  # noqa: F811
    for kernel in ("blur_quad_f16_norm_kernelILi0ELi128E", "blur_quad_f16_norm_kernelILi2ELi128E", "blur_quad_f16_norm_kernelILi0ELi256E",
                   "blur_quad_f16_norm_kernelILi2ELi256E"):
        r = _one(report, kernel)
        assert r["ScratchSize"] == 0 and r["Occupancy"] >= 8, (kernel, r)
