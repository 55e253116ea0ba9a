"""Register, scratch and LDS budget of the restoration-quality kernels (csrc/dib_restoration.hip), read from hipcc's own resource report, as
tests/test_quality_resources.py does for the single-pair kernels.  DESIGN.md section 4 states the occupancy the tile kernel is written
for: four workgroups of 256 lanes per CU = four waves per SIMD, which needs <= 128 vector registers per lane, <= 102 scalar registers per
wave and <= 160 KB / 4 of LDS per workgroup (sharp tile + its two planes + one candidate's three planes: 33,936 B, and 112 B of sums);
and no scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "detectinblur_amd", "csrc", "dib_restoration.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
WAVES_PER_SIMD = 4          # DESIGN.md section 4, "Restoration quality per sweep cell"
TILE_KERNELS = 4 + 8        # K = 1: <sharp, candidate>; K = 2: <sharp, candidate 0, candidate 1>, Half or fp32 each
LDS_BYTES = (42 * 42 + 5 * 42 * 32) * 4 + 8 * 8 + 12 * 4


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
    assert len(report) == TILE_KERNELS + 1, sorted(report)
    assert sum("restoration_tile_kernelILi1E" in n for n in report) == 4 and sum("restoration_tile_kernelILi2E" in n for n in report) == 8
    assert sum("restoration_finish_kernel" in n for n in report) == 1


def test_tile_kernels_have_no_scratch_and_the_stated_occupancy(report):
    tiles = {n: r for n, r in report.items() if "restoration_tile_kernel" in n}
    assert len(tiles) == TILE_KERNELS
    for n, r in tiles.items():
        assert r["ScratchSize"] == 0, (n, r)
        assert r["Occupancy"] >= WAVES_PER_SIMD and r["VGPRs"] <= 128 and r["TotalSGPRs"] <= 102, (n, r)
        assert r["LDS"] == LDS_BYTES and r["LDS"] * WAVES_PER_SIMD <= 160 * 1024, (n, r)


def test_the_final_sum_has_no_scratch(report):
    r = [v for n, v in report.items() if "restoration_finish_kernel" in n][0]
    assert r["ScratchSize"] == 0 and r["LDS"] == 2 * 256 * 8, r
