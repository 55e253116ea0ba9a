"""Register, scratch and LDS budget of the adversarial loss's kernels (csrc/dib_deblur_adv.hip), read from hipcc's own resource report as
tests/test_deblur_augment_resources.py does.  The LeakyReLU kernels are streams of one 16-byte vector per lane that hide their loads by
occupancy alone: the full 8 waves per SIMD, which needs at most 64 vector registers per lane; no scratch, no LDS.  The two loss kernels
reduce in LDS (256 floats) and use no scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "detectinblur_amd", "csrc", "dib_deblur_adv.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
WAVES_PER_SIMD = 8
# <L, MASK> of leaky_fwd_kernel and <L> of leaky_bwd_kernel as mangled
LEAKY = ["leaky_fwd_kernelINS_7F32LaneELb1EE", "leaky_fwd_kernelINS_7F32LaneELb0EE", "leaky_fwd_kernelINS_7F16LaneELb1EE",
         "leaky_fwd_kernelINS_7F16LaneELb0EE", "leaky_bwd_kernelINS_7F32LaneEEE", "leaky_bwd_kernelINS_7F16LaneEEE"]
# the loss's instantiations of csrc/dib_sliced_sum.h's two kernels as mangled
LOSS = ["sliced_sum_partial_kernelINS_7BceTermEEE", "sliced_sum_final_kernelINS_7BceTermEEE"]


@pytest.fixture(scope="module")
def report():
    if not os.path.isfile(HIPCC):
        pytest.skip("hipcc not available")
    p = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-c", SRC,
                        "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
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


def _one(report, kernel):
    names = [n for n in report if kernel in n]
    assert len(names) == 1, sorted(report)
    return report[names[0]]


def test_the_file_holds_exactly_the_eight_instantiations(report):
    assert len(report) == len(LEAKY) + len(LOSS), sorted(report)
    assert all(sum(k in n for n in report) == 1 for k in LEAKY + LOSS), sorted(report)


@pytest.mark.parametrize("kernel", LEAKY)
def test_leaky_kernels_no_scratch_no_lds_and_full_occupancy(report, kernel):
    r = _one(report, kernel)
    assert r["ScratchSize"] == 0 and r["LDS"] == 0, r
    assert r["VGPRs"] <= 64 and r["Occupancy"] >= WAVES_PER_SIMD, r


@pytest.mark.parametrize("kernel", LOSS)
def test_loss_kernels_use_no_scratch(report, kernel):
    assert _one(report, kernel)["ScratchSize"] == 0
