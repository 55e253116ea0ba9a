"""Register, scratch and LDS budget of the kernels the trainer's --amp step adds (the Half instantiations of bias_grad_partial_kernel in
csrc/dib_deblur_train.hip and the sign-mask forms of bias_act_kernel<F16Lane> in csrc/dib_eltwise_f16.hip), read from hipcc's own
resource report as tests/test_deconvolve_resources.py reads it: no scratch, eight waves per SIMD (<= 64 vector registers per lane, <= 80
scalar registers per wave), and LDS for eight workgroups per CU.  The fp32 instantiations of the kernel that was templated over its
storage keep the lines of profiles/deblur_train.txt, section 1."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "detectinblur_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
WAVES_PER_SIMD = 8
# bias_grad_partial_kernel<E, V, MASK, WRITE> as mangled: DF16_ = _Float16; masked, written without a mask, sum only
BIAS_GRAD_F16 = ["bias_grad_partial_kernelIDF16_Li8ELb1ELb1E", "bias_grad_partial_kernelIDF16_Li8ELb0ELb1E", "bias_grad_partial_kernelIDF16_Li8ELb0ELb0E",
                 "bias_grad_partial_kernelIDF16_Li1ELb1ELb1E", "bias_grad_partial_kernelIDF16_Li1ELb0ELb1E", "bias_grad_partial_kernelIDF16_Li1ELb0ELb0E"]
# <E, V, MASK, WRITE> -> (VGPRs, LDS bytes) of profiles/deblur_train.txt
BIAS_GRAD_F32 = {"bias_grad_partial_kernelIfLi4ELb1ELb1E": (23, 4096), "bias_grad_partial_kernelIfLi4ELb0ELb1E": (20, 4096),
                 "bias_grad_partial_kernelIfLi4ELb0ELb0E": (18, 4096), "bias_grad_partial_kernelIfLi1ELb0ELb1E": (12, 1024),
                 "bias_grad_partial_kernelIfLi1ELb0ELb0E": (12, 1024)}
# bias_act_kernel<F16Lane, RES, RELU = true, MASK = true>
BIAS_ACT_MASK_F16 = ["bias_act_kernelINS_7F16LaneELb0ELb1ELb1E", "bias_act_kernelINS_7F16LaneELb1ELb1ELb1E"]


def _report(source):
    if not os.path.isfile(HIPCC):
        pytest.skip("hipcc not available")
    p = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-c",
                        os.path.join(CSRC, source), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True,
                       timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    out, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    return out


@pytest.fixture(scope="module")
def train_report():
    return _report("dib_deblur_train.hip")


@pytest.fixture(scope="module")
def f16_report():
    return _report("dib_eltwise_f16.hip")


def _one(report, kernel):
    names = [n for n in report if kernel in n]
    assert len(names) == 1, sorted(report)
    return report[names[0]]


def _within_budget(r):
    assert r["ScratchSize"] == 0, r
    assert r["Occupancy"] >= WAVES_PER_SIMD and r["VGPRs"] <= 64 and r["TotalSGPRs"] <= 80, r
    assert r["LDS"] * WAVES_PER_SIMD <= 160 * 1024, r


@pytest.mark.parametrize("kernel", BIAS_GRAD_F16)
def test_half_bias_grad_kernels(train_report, kernel):
    _within_budget(_one(train_report, kernel))


@pytest.mark.parametrize("kernel", BIAS_ACT_MASK_F16)
def test_half_mask_epilogues(f16_report, kernel):
    r = _one(f16_report, kernel)
    _within_budget(r)
    assert r["LDS"] == 0, r


def test_fp32_bias_grad_kernels_are_what_they_were(train_report):
    assert sum("bias_grad_partial_kernel" in n for n in train_report) == 12, sorted(train_report)       # {fp32, Half} x {V, 1} x 3 forms
    for kernel, (vgprs, lds) in BIAS_GRAD_F32.items():
        r = _one(train_report, kernel)
        _within_budget(r)
        assert (r["VGPRs"], r["LDS"]) == (vgprs, lds), (kernel, r)
