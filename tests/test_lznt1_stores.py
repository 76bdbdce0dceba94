"""CPU: the stores of the LZNT1 chunk kernels as the compiler writes them for gfx950 (csrc/lznt1.hip, both translation units, the Makefile's
flags). Section D of the four-wave kernel stores through pointers whose address space the compiler knows (the slot's and the size index's addresses
come back from the parked lanes as integers and are cast to global pointers), so no FLAT instruction is left in any instance of either chunk
kernel: a FLAT store takes a 64-bit vector address and counts on lgkmcnt with the LDS reads. The listing is searched for that kind of instruction
alone. (The byte loads of section A's unaligned path are still there: staging with 16-byte loads at any alignment did not stand clear of its
predecessor on the MI355X and was not kept, profiles/HISTORY.md round 21.)"""
import functools
import os
import re
import subprocess
import tempfile

import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ms_compress_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
UNITS = pytest.mark.parametrize("extra", [(), ("-DLZNT1_DEV_TU",)], ids=["host-plans", "dev-plans"])
KERNELS = ("lznt1_chunk_kernel", "lznt1_chunk4_kernel")


def _makefile_flags():
    """HIPFLAGS of csrc/Makefile, with its ARCH and an empty EXTRA (as tests/test_lznt1_resources.py compiles the file)"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^HIPFLAGS\s*=\s*(.+)$", text, re.M).group(1)
    flags = flags.replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags, flags
    return flags


@functools.lru_cache(maxsize=None)
def _listing(extra):
    """{kernel symbol: [instruction lines]} of lznt1.hip's device code, one compile per translation unit"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "lznt1.s")
        subprocess.run([HIPCC] + _makefile_flags() + list(extra) + ["--cuda-device-only", "-S", os.path.join(CSRC, "lznt1.hip"), "-o", out],
                       capture_output=True, text=True, check=True)
        text = open(out).read()
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = kernels.setdefault(m.group(1), []) if any(k in m.group(1) for k in KERNELS) else None
            continue
        if cur is None:
            continue
        if line.startswith("\t.end_amdhsa_kernel") or re.match(r"^\s*\.section|^\s*\.rodata", line):
            cur = None
            continue
        m = re.match(r"^\s+([a-z][a-z0-9_]+)\b", line)
        if m and not line.lstrip().startswith("."):
            cur.append(line.strip())
    return kernels


@UNITS
def test_chunk_kernels_have_no_flat_access(extra):
    ks = _listing(extra)
    assert len(ks) == 4 and sum("chunk4" in k for k in ks) == 2, sorted(ks)     # serial / not serial of both kernels
    for name, ins in ks.items():
        assert len(ins) > 1000 and any(i.startswith("global_load_dwordx4") for i in ins) and any(i.startswith("global_store_") for i in ins), name
        flat = [i for i in ins if i.startswith("flat_")]
        print(name, len(ins), "instructions,", len(flat), "flat")
        assert not flat, (name, flat[:4])
