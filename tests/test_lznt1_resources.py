"""CPU: the resources of the four-wave LZNT1 chunk kernel as the compiler reports them for gfx950. The kernel is bound by vector
issue at 8 blocks (32 waves) per CU: it must stay within 20 480 B of LDS per block, 8 waves per SIMD, no scratch, no spills."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ms_compress_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _resources(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-exceptions", "-Wno-unused-function",
                          "-c", os.path.join(CSRC, "lznt1.hip"), "-o", str(tmp_path / "lznt1.o"), "-Rpass-analysis=kernel-resource-usage"],
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


def test_lznt1_chunk4_kernel_keeps_eight_blocks_per_cu(tmp_path):
    ks = _resources(tmp_path)
    four = [k for k in ks if "lznt1_chunk4_kernel" in k]
    one = [k for k in ks if "lznt1_chunk_kernel" in k]
    assert len(four) == 2 and len(one) == 2, sorted(ks)
    for name in four:
        r = ks[name]
        assert r["LDS Size"] <= 20480, (name, r)
        assert r["Occupancy"] == 8, (name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
    for name in one:                                     # (test-hook mode 1: within what it declares)
        assert ks[name]["LDS Size"] <= 65536 and ks[name]["ScratchSize"] == 0, (name, ks[name])
