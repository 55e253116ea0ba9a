"""Register, scratch and LDS budget of the patch-augmentation kernel (csrc/dib_deblur_augment.hip), read from hipcc's own resource report
as tests/test_quality_resources.py does.  A lane issues three dependent global loads and the kernel hides them by occupancy alone: it
is written for the full 8 waves per SIMD, which needs at most 64 vector registers per lane; and no scratch, no LDS."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "detectinblur_amd", "csrc", "dib_deblur_augment.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
WAVES_PER_SIMD = 8
# <T> of patches_augment_kernel as mangled: Half, fp32
INSTANTIATIONS = ["patches_augment_kernelI6__halfE", "patches_augment_kernelIfE"]


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


def test_the_file_holds_exactly_the_two_instantiations(report):
    assert len(report) == len(INSTANTIATIONS), sorted(report)
    assert all(sum(k in n for n in report) == 1 for k in INSTANTIATIONS), sorted(report)


@pytest.mark.parametrize("kernel", INSTANTIATIONS)
def test_no_scratch_no_lds_and_full_occupancy(report, kernel):
    names = [n for n in report if kernel in n]
    assert len(names) == 1, sorted(report)
    r = report[names[0]]
    assert r["ScratchSize"] == 0 and r["LDS"] == 0, r
    assert r["VGPRs"] <= 64 and r["Occupancy"] >= WAVES_PER_SIMD, r
