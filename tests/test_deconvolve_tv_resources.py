"""Register, scratch and LDS budget of the total-variation kernel (csrc/dib_deconv_tv.hip), read from hipcc's own resource report, as
tests/test_deconvolve_resources.py does for the two sweeps.  The file's header states what the kernel is written for: eight waves per
SIMD, which needs <= 64 vector registers per lane and <= 80 scalar registers per wave (81..96 silently run seven); no LDS at all -- a
wave shares its neighbours through lane shuffles and keeps its rows in registers -- and no scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "detectinblur_amd", "csrc", "dib_deconv_tv.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
WAVES_PER_SIMD = 8
# tv_weight_kernel<T> as mangled: x_0 = y in Half, every later x_k (and an fp32 y) in fp32
INSTANTIATIONS = ["tv_weight_kernelI6__halfE", "tv_weight_kernelIfE"]


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


def test_the_file_holds_the_tv_kernel_and_nothing_else(report):
    assert len(report) == len(INSTANTIATIONS) and all("tv_weight_kernel" in n for n in report), sorted(report)


@pytest.mark.parametrize("kernel", INSTANTIATIONS)
def test_the_kernel_has_no_scratch_no_lds_and_the_stated_occupancy(report, kernel):
    names = [n for n in report if kernel in n]
    assert len(names) == 1, sorted(report)
    r = report[names[0]]
    assert r["ScratchSize"] == 0, r
    assert r["LDS"] == 0, r
    assert r["Occupancy"] >= WAVES_PER_SIMD and r["VGPRs"] <= 64 and r["TotalSGPRs"] <= 80, r
