"""CPU: the interior-window copy of the four-wave LZNT1 kernel's window parse (csrc/lznt1.hip lz_window<true, true, true>, windows 1 to 62 of a
full chunk but 1, 2, 4, 8, 16 and 32) takes the token split, max_len and max_len << 12 from the window's base on the scalar unit, and its first
compare stage keeps no cap. The listing is compiled the way tests/test_lznt1_glue_listing.py compiles the file, and between the full-chunk
body's two markers of `lznt1_chunk4_kernel<false, false>`: one `v_ffbh_u32` less than the commit before (lz_shift's, one per window copy: the
interior copy has none and counts the leading zeros of the window's base with one `s_flbit_i32_b32`), and no `v_min_u32 64, ...` between the
interior copy's bucket lookup and its first key, where the commit before capped each of the four candidates' first-stage results."""
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
PARENT_FFBH = 4            # the commit before: one per window copy (cascade, speculative full-chunk, speculative interior, seam repair)
PARENT_CAPS = 4            # the commit before: `v_min_u32 vN, 64, vM` of the four candidates in the interior copy's first stage
_BODY = []


def _makefile_flags():
    """HIPFLAGS of csrc/Makefile, with its ARCH and an empty EXTRA (as tests/test_lznt1_full_listing.py compiles the file)"""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^HIPFLAGS\s*=\s*(.+)$", text, re.M).group(1)
    flags = flags.replace("$(ARCH)", arch).replace("$(EXTRA)", "").split()
    assert "--offload-arch=gfx950" in flags and "-O3" in flags, flags
    return flags


def _full_chunk_body():
    """the lines between the two markers of the full-chunk body inside lznt1_chunk4_kernel<false, false> (one compile for the file's tests)"""
    if _BODY:
        return _BODY[0]
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
    _BODY.append(kernel[b[0]:e[0]])
    return _BODY[0]


def _interior_first_stages(body):
    """The interior copy from its bucket lookup to its first key. The copy is the one that holds the body's only `s_flbit_i32_b32` (the split from
    the window's base), which lies between the copy's bucket lookup -- the last AND in front of it that aligns the packed table's dword address --
    and its walk, the first `s_bitcmp1_b64` behind it. The two compare stages lie between the lookup and the first `v_bitop3_b32` (lz_key) behind
    it: a cap of the first stage has to stand in front of the key that is made of its result."""
    at = [i for i, l in enumerate(body) if re.search(r"\bs_flbit_i32_b32\b", l)]
    assert len(at) == 1, at
    look = [i for i in range(at[0]) if re.search(r"\bv_and_b32_e32 v\d+, 0x1ffffffc, v\d+", body[i])]
    walk = [i for i in range(at[0], len(body)) if re.search(r"\bs_bitcmp1_b64\b", body[i])]
    assert look and walk
    keys = [i for i in range(look[-1], walk[0]) if re.search(r"\bv_bitop3_b32\b", body[i])]
    assert len(keys) == 4, keys                     # the four candidates' keys, between this copy's lookup and its walk
    return body[look[-1]:keys[0]]


def test_the_interior_copy_counts_no_leading_zeros_per_lane():
    body = _full_chunk_body()
    n = sum(1 for l in body if re.search(r"\bv_ffbh_u32\b", l))
    print("full-chunk body: %d lines, v_ffbh_u32 %d (the commit before: %d)" % (len(body), n, PARENT_FFBH))
    assert n == PARENT_FFBH - 1, n


def test_the_interior_copy_caps_no_first_stage():
    part = _interior_first_stages(_full_chunk_body())
    caps = [l.strip() for l in part if re.search(r"\bv_min_u32_e(32|64) v\d+, (64, v\d+|v\d+, 64)\s*$", l)]
    mins = [l for l in part if re.search(r"\bv_min_u32_e(32|64) v\d+, v\d+, v\d+\s*$", l)]
    ffbl = [l for l in part if re.search(r"\bv_ffbl_b32\b", l)]
    print("interior copy, bucket lookup to first key: %d lines, v_min_u32 of two registers %d, v_ffbl_b32 %d, v_min_u32 with 64: %d (the commit before: %d)"
          % (len(part), len(mins), len(ffbl), len(caps), PARENT_CAPS))
    # the first stage is there: four candidates, two v_ffbl_b32 and one plain minimum each; the second stage's eight v_ffbl_b32 behind it
    assert len(mins) >= 4 and len(ffbl) >= 16, (len(mins), len(ffbl))
    assert not caps, caps
    # the split is the window's: nothing of lz_shift in the copy's lanes
    assert not [l for l in part if re.search(r"\bv_ffbh_u32\b", l)]
