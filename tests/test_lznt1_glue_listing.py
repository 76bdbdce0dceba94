"""CPU: the window loops of the four-wave LZNT1 kernel's full-chunk body (csrc/lznt1.hip lz4_chunk_body<.., true>) write their control words --
a window's token and match mask, the parse position behind it, the repair flag, the segment's progress word -- behind the join of the window's
two arms, every lane storing the same value to the same address: no `lane == 0` region, so no exec mask is saved and restored around a store and
the "window already behind the position" test is a scalar compare and branch. The listing is compiled the way tests/test_lznt1_full_listing.py
compiles the file, and between the full-chunk body's two markers of `lznt1_chunk4_kernel<false, false>` the exec saves that guard a region
(`s_and_saveexec_b64` plus `s_andn2_saveexec_b64`) are counted: at most what the tree reached when the stores left their regions. What is left
belongs to per-lane work: the match-token record stores of the window copies, the finishing steps, the sort, the emission."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ms_compress_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNEL = "_ZN3msc19lznt1_chunk4_kernelILb0ELb0EEEvPKhNS_11BatchTablesEPhPjPt"
BEGIN, END = "; lznt1 full-chunk body begins", "; lznt1 full-chunk body ends"
PARENT_SAVES = 54          # the commit before: 52 s_and_saveexec_b64 and 2 s_andn2_saveexec_b64, three window copies with three lane-0 regions each
MAX_SAVES = 41             # this tree: 41 and 0, four window copies (the interior-window copy of the speculative loop is the fourth)


def _makefile_flags():
    """HIPFLAGS of csrc/Makefile, with its ARCH and an empty EXTRA (as tests/test_lznt1_full_listing.py compiles the file)"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^HIPFLAGS\s*=\s*(.+)$", text, re.M).group(1)
    flags = flags.replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags, flags
    return flags


def _full_chunk_body():
    """the lines between the two markers of the full-chunk body inside lznt1_chunk4_kernel<false, false>"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "lznt1.s")
        subprocess.run([HIPCC] + _makefile_flags() + ["--cuda-device-only", "-S", os.path.join(CSRC, "lznt1.hip"), "-o", out],
                       capture_output=True, text=True, check=True)
        lines = open(out).read().splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith(KERNEL + ":"))
    stop = next(i for i in range(start, len(lines)) if lines[i].lstrip().startswith(".amdhsa_kernel"))
    kernel = lines[start:stop]
    b = [i for i, l in enumerate(kernel) if BEGIN in l]
    e = [i for i, l in enumerate(kernel) if END in l]
    assert len(b) == 1 and len(e) == 1 and b[0] < e[0], (b, e)
    return kernel[b[0]:e[0]]


def test_the_window_loops_store_their_control_words_outside_exec_regions():
    body = _full_chunk_body()
    n_and = sum(1 for l in body if re.search(r"\bs_and_saveexec_b64\b", l))
    n_andn2 = sum(1 for l in body if re.search(r"\bs_andn2_saveexec_b64\b", l))
    print("full-chunk body: %d lines, s_and_saveexec_b64 %d, s_andn2_saveexec_b64 %d (the commit before: %d together)" % (len(body), n_and, n_andn2, PARENT_SAVES))
    assert MAX_SAVES < PARENT_SAVES
    assert n_and + n_andn2 <= MAX_SAVES, (n_and, n_andn2)
    # the control words' stores are there, one sequence per window copy: two 8-byte mask stores each
    assert sum(1 for l in body if re.search(r"\bds_write_b64\b", l)) >= 6
