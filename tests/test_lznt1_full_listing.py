"""CPU: the four-wave LZNT1 kernel holds two bodies behind one branch (csrc/lznt1.hip: the full-chunk body and the body for any length), inside
the kernels the file always had. The listing is compiled the way tests/test_lznt1_resources.py compiles the file (the Makefile's flags, one
compile per translation unit) and two things are checked: each translation unit holds exactly the kernel symbols it held before the second body
came -- bench.py looks `lznt1_chunk4_kernel<false>` up by name and the resource test counts the instances -- and the code of
`lznt1_chunk4_kernel<false, false>`, which grew by the second copy, stays below 65 536 bytes."""
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
MAX_CODE = 65536
# <serial, DEV> of the one-wave and the four-wave kernel: the host-plan unit holds DEV = false, the device-plan unit DEV = true
SYMBOLS = {(): ["_ZN3msc18lznt1_chunk_kernelILb0ELb0EEEvPKhNS_11BatchTablesEPhPj", "_ZN3msc18lznt1_chunk_kernelILb1ELb0EEEvPKhNS_11BatchTablesEPhPj",
                "_ZN3msc19lznt1_chunk4_kernelILb0ELb0EEEvPKhNS_11BatchTablesEPhPjPt", "_ZN3msc19lznt1_chunk4_kernelILb1ELb0EEEvPKhNS_11BatchTablesEPhPjPt"],
           ("-DLZNT1_DEV_TU",): ["_ZN3msc18lznt1_chunk_kernelILb0ELb1EEEvPKhNS_11BatchTablesEPhPj", "_ZN3msc18lznt1_chunk_kernelILb1ELb1EEEvPKhNS_11BatchTablesEPhPj",
                                 "_ZN3msc19lznt1_chunk4_kernelILb0ELb1EEEvPKhNS_11BatchTablesEPhPjPt", "_ZN3msc19lznt1_chunk4_kernelILb1ELb1EEEvPKhNS_11BatchTablesEPhPjPt"]}
UNITS = pytest.mark.parametrize("extra", list(SYMBOLS), ids=["host-plans", "dev-plans"])


def _makefile_flags():
    """HIPFLAGS of csrc/Makefile, with its ARCH and an empty EXTRA (as tests/test_lznt1_resources.py compiles the file)"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^HIPFLAGS\s*=\s*(.+)$", text, re.M).group(1)
    flags = flags.replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags, flags
    return flags


@functools.lru_cache(maxsize=None)
def _kernels(extra):
    """{kernel symbol: codeLenInByte} of the device code of lznt1.hip, one compile per translation unit"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "lznt1.s")
        subprocess.run([HIPCC] + _makefile_flags() + list(extra) + ["--cuda-device-only", "-S", os.path.join(CSRC, "lznt1.hip"), "-o", out],
                       capture_output=True, text=True, check=True)
        text = open(out).read()
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.match(r"^;\s*codeLenInByte\s*=\s*(\d+)", line)
        if m and cur is not None:
            kernels[cur] = int(m.group(1))
            cur = None
    return kernels


@UNITS
def test_the_unit_holds_the_kernels_it_always_held(extra):
    ks = _kernels(extra)
    print(ks)
    assert sorted(ks) == sorted(SYMBOLS[extra]), sorted(ks)


def test_the_two_bodies_fit_the_code_limit():
    name = "_ZN3msc19lznt1_chunk4_kernelILb0ELb0EEEvPKhNS_11BatchTablesEPhPjPt"
    size = _kernels(())[name]
    print(name, "codeLenInByte", size)
    assert 0 < size < MAX_CODE, size
