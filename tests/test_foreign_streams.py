"""CPU: streams that no encoder writes (tests/streams.py), put to the checker and to the compiled reference.

The writer's self-check: every valid stream decodes in the checker to the writer's plaintext at the smallest capacity that holds it, and
every family holds the features it is there for (counted while the writer wrote them). Then the checker against the compiled reference on
every stream, status and bytes: one question per family (tests/refanswers.py), whose answer is the digest of the list of per-stream results.
"""
import pytest

import streams
from refanswers import answer, digest

FMTS = {"lznt1": 2, "xpress": 3, "xpress_huff": 4}
FEATURES = {   # counted in streams.STATS while a family is written: each must occur
    2: ["lznt1 offset to the chunk start", "lznt1 largest length at a split", "lznt1 payload of 4096 bytes", "lznt1 payload longer than its output",
        "lznt1 short compressed chunk in the middle", "lznt1 stored chunk in the middle", "lznt1 full chunk with flag bits left",
        "lznt1 end '00'", "lznt1 end '0'", "lznt1 end ''"],
    3: ["xpress 16-bit length below 280", "xpress 32-bit length below 65536", "xpress 32-bit length that wraps", "xpress length nibble never used",
        "xpress offset 1", "xpress offset 2", "xpress offset 3", "xpress offset 8192", "xpress overlapping match"],
    4: ["xpress_huff incomplete code", "xpress_huff 15-bit code length", "xpress_huff one-symbol code", "xpress_huff code without 0x100",
        "xpress_huff 0x100 as a match", "xpress_huff offset 65535", "xpress_huff 16-bit length below 270", "xpress_huff 32-bit length below 65536",
        "xpress_huff 32-bit length that wraps", "xpress_huff chunk that starts off the grid", "xpress_huff token read past the mark"]
        + ["xpress_huff offset bits %d" % b for b in range(16)],
}
TAGS = {       # tags of the families' streams: each must be there
    2: ["nongreedy", "multi_segment", "variant_short", "variant_long", "variant_cap_short", "variant_cap_exact"],
    3: ["len_form_None", "len_form_16", "len_form_32", "end_flags_legal", "end_flags_illegal", "short", "four_byte", "five_byte", "large_input", "len32_nowrap",
        "variant_short", "variant_long", "variant_cap_short"],
    4: ["complete", "incomplete", "xlen32_nowrap", "on_grid", "big_complete", "big_incomplete", "variant_short", "variant_long", "variant_cap_short"],
}

_families = {}


def family(f):
    """the streams of format f (generated once per process), and the feature counts their writing produced"""
    if f not in _families:
        before = streams.STATS.copy()
        fam = streams.FAMILIES[f]()
        _families[f] = (fam, streams.STATS - before)
    return _families[f]


def checker_results(oracle, f, fam):
    """[(status, bytes)] of the checker for every stream, and the indices of the streams the reference is not asked about (undefined)"""
    res, undefined = [], set()
    for i, s in enumerate(fam):
        st, out, und = oracle.oracle_decompress_ex(f, s.data, s.cap)
        res.append((st, out if st == 0 else b""))
        if und:
            undefined.add(i)
    return res, undefined


def reference_answer(oracle, f, fam, undefined):
    """the compiled reference's answer for the family: the digest of [(status, bytes)] over its defined streams (live, or as recorded)"""
    asked = [(s.data, s.cap) for i, s in enumerate(fam) if i not in undefined]
    ref = oracle.load_ref()
    return answer(("foreign streams", f, digest(asked)), ref and (lambda: [oracle.ref_decompress(f, d, c) for d, c in asked]))


def first_difference(oracle, f, fam, undefined, mine):
    """where the live reference is present: the first stream on which it and `mine` disagree"""
    if oracle.load_ref() is None:
        return "(no live reference to point at the stream)"
    for i, s in enumerate(fam):
        if i in undefined:
            continue
        r = oracle.ref_decompress(f, s.data, s.cap)
        if r != mine[i]:
            return "stream %d %s (%d bytes, capacity %d): reference %s / %d bytes, here %s / %d bytes" % (
                i, sorted(s.tags), len(s.data), s.cap, r[0], len(r[1]), mine[i][0], len(mine[i][1]))
    return "(no single stream differs)"


@pytest.mark.parametrize("fmt", list(FMTS))
def test_writer_streams_decode_in_the_checker(oracle, fmt):
    f = FMTS[fmt]
    fam, stats = family(f)
    n_valid = 0
    for i, s in enumerate(fam):
        if s.plain is None:
            continue
        st, out, und = oracle.oracle_decompress_ex(f, s.data, s.cap)
        assert (st, und) == (0, False) and out == s.plain, (i, sorted(s.tags), st, len(out), len(s.plain))
        n_valid += 1
    assert n_valid > 20
    counts = {k: stats[k] for k in FEATURES[f]}
    assert all(counts.values()), counts
    tags = {t: sum(t in s.tags for s in fam) for t in TAGS[f]}
    assert all(tags.values()), tags


def test_feature_structure():
    """features read back from the bytes: the large Xpress input, and the multi-MB Xpress+Huffman buffers: 40 chunks or more, every code
    complete in some, exactly one incomplete in the others"""
    fam, _ = family(3)
    assert max(len(s.data) for s in fam if "large_input" in s.tags) >= 512 << 10
    fam, _ = family(4)
    big = [s for s in fam if "big" in s.tags]
    assert len(big) == 4 and all(len(s.plain) >= 2 << 20 for s in big), [len(s.plain) for s in big]
    assert {s.tags for s in big} >= {frozenset({"big", "big_complete", "off_grid"}), frozenset({"big", "big_incomplete", "off_grid"})}
    for s in big:
        tables = [streams.kraft([(b >> (4 * h)) & 0xF for b in s.data[p: p + 256] for h in (0, 1)]) for p in chunk_starts(s.data, len(s.plain))]
        assert len(tables) >= 40 and tables.count(32768) >= len(tables) - ("big_incomplete" in s.tags), len(tables)
        assert ("big_incomplete" in s.tags) == (min(tables) < 32768)


def chunk_starts(data, cap):
    """input offsets of the chunks of an Xpress+Huffman stream, by the checker's walk"""
    import ctypes as C
    import numpy as np
    from oracle import loader
    lib = loader.load_oracle()
    lib.orc_xh_chunk_starts.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t]
    lib.orc_xh_chunk_starts.restype = C.c_long
    starts = np.zeros(4096, np.uint64)
    n = lib.orc_xh_chunk_starts(bytes(data), len(data), cap, starts.ctypes.data, len(starts))
    assert 0 < n <= len(starts)
    return [int(x) for x in starts[:n]]


@pytest.mark.parametrize("fmt", list(FMTS))
def test_checker_answers_like_the_reference(oracle, fmt):
    """status and bytes of every stream of the family, invalid variants included (streams on which the reference is undefined are not put to it)"""
    f = FMTS[fmt]
    fam, _ = family(f)
    mine, undefined = checker_results(oracle, f, fam)
    assert len(undefined) < len(fam) // 10
    want = reference_answer(oracle, f, fam, undefined)
    got = digest([r for i, r in enumerate(mine) if i not in undefined])
    assert got == want, first_difference(oracle, f, fam, undefined, mine)
