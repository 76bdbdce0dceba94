"""CPU: the register budget of the four-wave LZNT1 chunk kernel. The hardware hands scalar registers out in sixteens, 800 per SIMD: at 96 eight
blocks fit a CU, the 97th register costs the eighth block (5 to 7 % of the headline, round 13 in profiles/HISTORY.md), while the compiler's own
occupancy figure still says 8 up to 100 -- so tests/test_lznt1_resources.py cannot see it. This test reads the counts themselves, for the four
instances of lznt1_chunk4_kernel: the two of lznt1.hip compiled with the Makefile's flags, and the two of the device-table plans
(lznt1_dev.hip: the same file with LZNT1_DEV_TU defined)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ms_compress_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
MAX_SGPRS, MAX_VGPRS = 96, 64


def _makefile_flags():
    """HIPFLAGS of csrc/Makefile, with its ARCH and an empty EXTRA"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^HIPFLAGS\s*=\s*(.+)$", text, re.M).group(1)
    flags = flags.replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags, flags
    return flags


def _registers(tmp_path, extra):
    """{kernel name: {remark: value}} of lznt1.hip's kernels"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = subprocess.run([HIPCC] + _makefile_flags() + extra + ["-c", os.path.join(CSRC, "lznt1.hip"), "-o", str(tmp_path / "lznt1.o"),
                                                                "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, check=True).stderr
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return kernels


@pytest.mark.parametrize("extra", [[], ["-DLZNT1_DEV_TU"]], ids=["host-plans", "dev-plans"])
def test_lznt1_chunk4_kernel_register_budget(tmp_path, extra):
    ks = _registers(tmp_path, extra)
    four = sorted(k for k in ks if "lznt1_chunk4_kernel" in k)
    assert len(four) == 2, sorted(ks)                      # serial / not serial
    for name in four:
        r = ks[name]
        print(name, "TotalSGPRs", r["TotalSGPRs"], "VGPRs", r["VGPRs"])
        assert r["TotalSGPRs"] <= MAX_SGPRS, (name, r)
        assert r["VGPRs"] <= MAX_VGPRS, (name, r)
