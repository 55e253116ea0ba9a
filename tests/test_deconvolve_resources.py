"""Register, scratch and LDS budget of the Richardson-Lucy sweep kernels (csrc/dib_deconv.hip), read from hipcc's own resource report,
as tests/test_kernel_resources.py does for the blur.  DESIGN.md section 4 states the occupancy these kernels are written for: eight
workgroups of 256 lanes per CU = eight waves per SIMD, which needs <= 64 vector registers per lane, <= 80 scalar registers per wave
(81..96 silently run seven) and <= 160 KB / 8 of LDS per workgroup; and no scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "detectinblur_amd", "csrc", "dib_deconv.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
WAVES_PER_SIMD = 8          # DESIGN.md section 4, "--deconvolve_first"
# <ADJ, S, E> of rl_sweep_kernel as mangled: sweep A (Lb0) on y itself, on x_k with Half y, all fp32; sweep A* (Lb1) with x_0 = y, with x_k
INSTANTIATIONS = ["rl_sweep_kernelILb0E6__halfS2_E", "rl_sweep_kernelILb0Ef6__halfE", "rl_sweep_kernelILb0EffE",
                  "rl_sweep_kernelILb1Ef6__halfE", "rl_sweep_kernelILb1EffE"]


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


def test_the_file_holds_the_two_sweeps_and_nothing_else(report):
    assert len(report) == len(INSTANTIATIONS) and all("rl_sweep_kernel" in n for n in report), sorted(report)
    assert any("ILb0E" in n for n in report) and any("ILb1E" in n for n in report)      # sweep A and sweep A*


@pytest.mark.parametrize("kernel", INSTANTIATIONS)
def test_sweeps_have_no_scratch_and_the_stated_occupancy(report, kernel):
    names = [n for n in report if kernel in n]
    assert len(names) == 1, sorted(report)
    r = report[names[0]]
    assert r["ScratchSize"] == 0, r
    assert r["Occupancy"] >= WAVES_PER_SIMD and r["VGPRs"] <= 64 and r["TotalSGPRs"] <= 80, r
    assert r["LDS"] * WAVES_PER_SIMD <= 160 * 1024, r
