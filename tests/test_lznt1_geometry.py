"""CPU: the geometry that tests/lznt1_model.py states -- and the LZNT1 case files aim their units by -- is the geometry csrc/lznt1.hip is built with.
The kernel source is read as text: the default value of every #define the model mirrors, lz_hash's multiplier, and LZNT1_REC of kernels.h."""
import os
import re

import lznt1_model as M

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ms_compress_amd", "csrc")


def _define(text, name):
    m = re.search(r"^\s*#\s*define\s+%s\s+(\d+)u?\b" % name, text, re.M)
    assert m, "no #define of %s with a plain number" % name
    return int(m.group(1))


def test_the_model_has_the_kernels_geometry():
    hip = open(os.path.join(CSRC, "lznt1.hip")).read()
    stale = "csrc/lznt1.hip has %s = %d: %s of tests/lznt1_model.py is stale, and the LZNT1 case files aim at the wrong positions"
    model = {"LZ_TBL_BITS": ("BITS", M.BITS), "LZ_SELF": ("SELF", M.SELF), "LZ4_MAXM": ("MAXM", M.MAXM),
             "LZ4_P1": ("PART_FIRST[1] / 64", M.PART_FIRST[1] // 64), "LZ4_P2": ("PART_FIRST[2] / 64", M.PART_FIRST[2] // 64),
             "LZ4_B1": ("SEG_FIRST_WINDOW[1]", M.SEG_FIRST_WINDOW[1]), "LZ4_B2": ("SEG_FIRST_WINDOW[2]", M.SEG_FIRST_WINDOW[2]),
             "LZ4_B3": ("SEG_FIRST_WINDOW[3]", M.SEG_FIRST_WINDOW[3]), "LZ4_NSEG": ("len(SEG_FIRST_WINDOW) - 1", len(M.SEG_FIRST_WINDOW) - 1)}
    for name, (what, value) in model.items():
        got = _define(hip, name)
        assert got == value, stale % (name, got, what)
    assert M.PART_FIRST[0] == 0 and all(p % 64 == 0 for p in M.PART_FIRST), "PART_FIRST: parts start at batches of 64 positions"
    assert M.SEG_FIRST_WINDOW[0] == 0 and 64 * M.SEG_FIRST_WINDOW[-1] == M.CHUNK, "SEG_FIRST_WINDOW: from window 0 to the chunk's end"
    m = re.search(r"\blz_hash\s*\([^)]*\)\s*\{[^}]*?\*\s*0x([0-9A-Fa-f]+)u?\s*\)\s*>>\s*\(\s*32\s*-\s*LZ_TBL_BITS\s*\)", hip)
    assert m, "lz_hash is no longer a multiplication shifted right by 32 - LZ_TBL_BITS: raw_hash of tests/lznt1_model.py is stale"
    assert int(m.group(1), 16) == M.HASH_MUL, "lz_hash multiplies by 0x%s: HASH_MUL of tests/lznt1_model.py is stale" % m.group(1)
    rec = _define(open(os.path.join(CSRC, "kernels.h")).read(), "LZNT1_REC")
    assert rec == 2 * 64 * M.MAXM * 2, "kernels.h has LZNT1_REC = %d, MAXM of tests/lznt1_model.py gives %d: one of them is stale" % (rec, 2 * 64 * M.MAXM * 2)
