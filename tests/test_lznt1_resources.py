"""CPU: the resources of the four-wave LZNT1 chunk kernel as the compiler reports them for gfx950. The kernel is bound by vector issue at
8 blocks (32 waves) per CU: it must stay within 20 480 B of LDS per block, 64 vector registers, no scratch, no spills -- and within the scalar
registers of eight blocks. A SIMD has 800 of them and a wave is given its count rounded up to a multiple of 16, plus 16:

    blocks of 256 threads per CU = min(8, floor(800 / (ceil(TotalSGPRs / 16) * 16 + 16)))

so up to 80 registers make 8 blocks, 81 to 96 make 7 and 97 to 112 make 6, while the compiler's own occupancy figure says 8 up to 100. An
earlier limit of 96 was therefore the limit of SEVEN blocks (rounds 7 to 14 ran at seven, profiles/HISTORY.md round 15); the limit here is the
eight-block one, for the four instances of lznt1_chunk4_kernel: the two of lznt1.hip compiled with the Makefile's flags and the two of the
device-table plans (lznt1_dev.hip: the same file with LZNT1_DEV_TU defined). Each of the two translation units is compiled once."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ms_compress_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
MAX_SGPRS, MAX_VGPRS, MAX_LDS = 80, 64, 20480
UNITS = pytest.mark.parametrize("extra", [(), ("-DLZNT1_DEV_TU",)], ids=["host-plans", "dev-plans"])


def blocks_per_cu(sgprs):
    """what the scalar registers admit"""
    return min(8, 800 // ((sgprs + 15) // 16 * 16 + 16))


def test_formula():
    assert [blocks_per_cu(s) for s in (77, 80, 81, 93, 96, 97, 112)] == [8, 8, 7, 7, 7, 6, 6]


def _makefile_flags():
    """HIPFLAGS of csrc/Makefile, with its ARCH and an empty EXTRA"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^HIPFLAGS\s*=\s*(.+)$", text, re.M).group(1)
    flags = flags.replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags, flags
    return flags


@functools.lru_cache(maxsize=None)
def _resources(extra):
    """{kernel name: {remark: value}} of lznt1.hip's kernels, compiled once per translation unit"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([HIPCC] + _makefile_flags() + list(extra) + ["-c", os.path.join(CSRC, "lznt1.hip"), "-o", os.path.join(tmp, "lznt1.o"),
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


@UNITS
def test_lznt1_chunk4_kernel_fits_eight_blocks(extra):
    ks = _resources(extra)
    four = sorted(k for k in ks if "lznt1_chunk4_kernel" in k)
    assert len(four) == 2, sorted(ks)                      # serial / not serial
    for name in four:
        r = ks[name]
        print(name, {k: r[k] for k in ("TotalSGPRs", "VGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "LDS Size", "Occupancy")})
        assert r["TotalSGPRs"] <= MAX_SGPRS and blocks_per_cu(r["TotalSGPRs"]) == 8, (name, r)
        assert r["VGPRs"] <= MAX_VGPRS, (name, r)
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["ScratchSize"] == 0, (name, r)
        assert r["LDS Size"] <= MAX_LDS, (name, r)
        assert r["Occupancy"] == 8, (name, r)


def test_lznt1_chunk4_kernel_keeps_eight_blocks_per_cu():
    """the host-plan unit also holds the one-wave kernel of test-hook mode 1: within what it declares"""
    ks = _resources(())
    one = [k for k in ks if "lznt1_chunk_kernel" in k]
    assert len(one) == 2, sorted(ks)
    for name in one:
        assert ks[name]["LDS Size"] <= 65536 and ks[name]["ScratchSize"] == 0, (name, ks[name])
