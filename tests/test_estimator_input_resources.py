"""Compiler only: every instantiation of the input epilogue (csrc/dib_epilogue.hip) -- the zero-padded batch, and the cropped and
quantising forms the estimator's input added -- is one thread per output pixel with no scratch and no LDS."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_epilogue_kernels_use_no_scratch_and_no_lds():
    if not os.path.isfile(HIPCC):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "detectinblur_amd", "csrc", "dib_epilogue.hip")
    p = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-c", src,
                        "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    out, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    resize = [n for n in out if "normalize_resize_pad_kernel" in n]
    # T x layout x contraction x crop, and the quantising forms for fp16 only: 16 + 8
    assert len(resize) == 24, sorted(resize)
    assert len([n for n in out if "normalize_pad_kernel" in n]) == 4
    for n in resize + [n for n in out if "normalize_pad_kernel" in n]:
        assert out[n]["ScratchSize"] == 0 and out[n]["LDS"] == 0, (n, out[n])
        assert out[n]["Occupancy"] >= 4, (n, out[n])
