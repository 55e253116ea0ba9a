"""Register, scratch and LDS budget of the image-quality kernels (csrc/dib_quality.hip), read from hipcc's own resource report, as
tests/test_deconvolve_resources.py does for the Richardson-Lucy sweeps.  DESIGN.md section 4 states the occupancy the tile kernel is
written for: four workgroups of 256 lanes per CU = four waves per SIMD, which needs <= 128 vector registers per lane, <= 102 scalar
registers per wave and <= 160 KB / 4 of LDS per workgroup; and no scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "detectinblur_amd", "csrc", "dib_quality.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
WAVES_PER_SIMD = 4          # DESIGN.md section 4, "Restoration quality"
# <TA, TB> of quality_tile_kernel as mangled: Half / Half, Half / fp32, fp32 / Half, fp32 / fp32
INSTANTIATIONS = ["quality_tile_kernelI6__halfS2_E", "quality_tile_kernelI6__halffE", "quality_tile_kernelIf6__halfE", "quality_tile_kernelIffE"]


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


def test_the_file_holds_the_tile_kernels_and_the_final_sum(report):
    assert len(report) == len(INSTANTIATIONS) + 1, sorted(report)
    assert sum("quality_tile_kernel" in n for n in report) == len(INSTANTIATIONS) and sum("quality_finish_kernel" in n for n in report) == 1


@pytest.mark.parametrize("kernel", INSTANTIATIONS)
def test_tile_kernels_have_no_scratch_and_the_stated_occupancy(report, kernel):
    names = [n for n in report if kernel in n]
    assert len(names) == 1, sorted(report)
    r = report[names[0]]
    assert r["ScratchSize"] == 0, r
    assert r["Occupancy"] >= WAVES_PER_SIMD and r["VGPRs"] <= 128 and r["TotalSGPRs"] <= 102, r
    assert r["LDS"] * WAVES_PER_SIMD <= 160 * 1024, r


def test_the_final_sum_has_no_scratch(report):
    r = [v for n, v in report.items() if "quality_finish_kernel" in n][0]
    assert r["ScratchSize"] == 0 and r["LDS"] == 2 * 256 * 8, r
