"""hipcc's resource report of one csrc file, for the tests that hold its kernels to a register and scratch budget."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

_REPORTS = {}


def kernel_resources(source):
    """{mangled kernel name: {"ScratchSize": bytes per lane, "Occupancy": waves per SIMD}} of detectinblur_amd/csrc/`source`,
    compiled for gfx950 with the library's code-generation flags; one compilation per file and process.  Skips the calling test
    where there is no hipcc."""
    if not os.path.isfile(HIPCC):
        pytest.skip("hipcc not available")
    if source not in _REPORTS:
        src = os.path.join(ROOT, "detectinblur_amd", "csrc", source)
        p = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-c", src,
                            "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        out, cur = {}, None
        for line in p.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(m.group(1), {})
                continue
            m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
            if m and cur is not None:
                cur[m.group(1).split(" ")[0]] = int(m.group(2))
        _REPORTS[source] = out
    return _REPORTS[source]
