"""The class rules of the block transcoder (include/mscomp_amd.h) give mscomp_amd_blocks_compress's bytes: tests/transcode_model.py against
blocks_model.model_compress + crc_model at the new format and block size, on the CPU. This is the proof that carrying is sound -- an LZNT1
block is the concatenation of its chunks' images --, so a case that fails here is fixed in the header's rule, not in this test."""
import functools

import numpy as np
import pytest

import blocks_model as M
import thresholds as T
import transcode_model as X
from oracle import loader

LZNT1, XPRESS, XHUFF = 2, 3, 4
LZ_PAIRS = [(LZNT1, b1, LZNT1, b2) for b1 in M.BLOCK_SIZES for b2 in M.BLOCK_SIZES if b1 != b2]
CROSS = [(LZNT1, 4096, XHUFF, 32768), (XPRESS, 65536, LZNT1, 4096), (XPRESS, 32768, XPRESS, 65536)]


@functools.lru_cache(maxsize=None)
def recipe_buffers(B):
    """the fixture's recipes at block size B (threshold recipes: the LZNT1 ones of this size, and the short lone blocks)"""
    fx = M.load()
    return tuple(M.build(r, B) for r in M.recipes_for(fx, LZNT1, B))


@functools.lru_cache(maxsize=None)
def threshold_buffers():
    """the LZNT1 entries of tests/golden/thresholds.json: chunks whose compressed image is n or n + 1 bytes sit among them"""
    return tuple(T.build(c) for c in T.load()["cases"] if c["codec"] == "lznt1")


def edge_buffers(B2):
    rs = np.random.RandomState(B2)
    return tuple(M._text(rs, n) for n in (0, 1, 4095, 4096, 4097, B2 - 1, B2 + 1))


def check(f1, B1, f2, B2, bufs, with_crc):
    bufs = list(bufs)
    lens = [len(b) for b in bufs]
    packed, first, off, crc = X.fresh(loader, f1, bufs, B1, with_crc)
    want_packed, want_first, want_off, want_crc = X.fresh(loader, f2, bufs, B2, with_crc)
    nbt, nbn, G = len(off) - 1, len(want_off) - 1, max(B1, B2)
    groups = sum((n + G - 1) // G for n in lens)
    got = X.transcode(loader, f1, B1, f2, B2, packed, len(packed), first, off, lens, crc, nbt, nbn, groups, sum(lens))
    new_packed, new_first, new_off, new_crc, status, counts = got
    assert [int(s) for s in status] == [M.OK] * len(bufs)
    assert [int(x) for x in new_first] == [int(x) for x in want_first]
    assert [int(x) for x in new_off] == [int(x) for x in want_off]
    assert new_packed == want_packed
    if with_crc:
        assert [int(x) for x in new_crc] == [int(x) for x in want_crc]
    else:
        assert new_crc is None
    assert counts[0] + counts[2] <= nbn and counts[1] <= nbt
    return counts, nbn


@pytest.mark.parametrize("with_crc", [False, True], ids=["plain", "crc"])
@pytest.mark.parametrize("pair", LZ_PAIRS + CROSS, ids=lambda p: "%d-%d-to-%d-%d" % p)
def test_recipes(pair, with_crc):
    """the recipes of tests/golden/blocks.json built at the coarser block size of the pair (at 65536 for 524288: the whole 512 KiB blocks are
    test_large_block_recipes'): every family lands on both sizes' boundaries"""
    f1, B1, f2, B2 = pair
    counts, nbn = check(f1, B1, f2, B2, recipe_buffers(min(max(B1, B2), 65536)), with_crc)
    if f1 == f2 == LZNT1:
        assert counts[0] > 0                                   # text and zeros are carried
        if B2 < B1:
            assert counts[2] > 0 or not with_crc               # raw-stored source blocks are encoded, nothing else is
    else:
        assert counts[0] == 0 and counts[2] == nbn


@pytest.mark.parametrize("with_crc", [False, True], ids=["plain", "crc"])
@pytest.mark.parametrize("pair", LZ_PAIRS, ids=lambda p: "%d-%d-to-%d-%d" % p)
def test_threshold_chunks(pair, with_crc):
    """chunks whose image is as long as the chunk, or a byte longer: stored raw at 4096 although the encoder did not fall back; carried
    inside a larger block whose other chunks shrink"""
    f1, B1, f2, B2 = pair
    check(f1, B1, f2, B2, threshold_buffers(), with_crc)


@pytest.mark.parametrize("pair", LZ_PAIRS + CROSS, ids=lambda p: "%d-%d-to-%d-%d" % p)
def test_edge_lengths(pair):
    f1, B1, f2, B2 = pair
    check(f1, B1, f2, B2, edge_buffers(B2), True)


def test_large_block_recipes():
    """the recipes at 524288: whole 512 KiB blocks joined from, and split into, 4 KiB ones"""
    bufs = [b for b in recipe_buffers(524288) if len(b) <= 524288 + 7][:8]
    for B1, B2 in ((4096, 524288), (524288, 4096)):
        check(LZNT1, B1, LZNT1, B2, bufs, True)


def test_split_counts_decoded_once_stored_raw():
    """a 64 KiB block by turns random and text at 4 KiB: compressed-stored as a whole, its random chunks do not shrink alone -- decoded
    once, those new blocks stored raw, nothing encoded"""
    rs = np.random.RandomState(5)
    buf = b"".join(rs.bytes(4096) if i % 4 == 0 else M._text(rs, 4096) for i in range(16))
    counts, nbn = check(LZNT1, 65536, LZNT1, 4096, [buf], False)
    assert counts == (12, 1, 0) and nbn == 16


def test_rules_in_order():
    rs = np.random.RandomState(9)
    bufs = [M._text(rs, 4 * 4096), rs.bytes(2 * 4096), M._text(rs, 8192)]
    lens = [len(b) for b in bufs]
    packed, first, off, crc = X.fresh(loader, LZNT1, bufs, 4096, True)
    nbt = len(off) - 1
    args = (loader, LZNT1, 4096, LZNT1, 8192, packed, len(packed))
    # rule 0
    bad_first = first.copy(); bad_first[1] = first[2] + 1
    got = X.transcode(*args, bad_first, off, lens, crc, nbt, 5, 5, sum(lens))
    assert list(got[4]) == [M.ARG] * 3 and not got[1].any() and not got[2].any() and got[5] == (0, 0, 0)
    # rule 1: one resource's length says another block count
    got = X.transcode(*args, first, off, [lens[0] + 4096, lens[1], lens[2]], crc, nbt, 5, 5, sum(lens))
    assert list(got[4]) == [M.DATA, M.OK, M.OK] and list(got[1]) == [0, 0, 1, 2]
    # rule 2: the new table one row short
    got = X.transcode(*args, first, off, lens, crc, nbt, 3, 5, sum(lens))
    assert list(got[4]) == [M.OK, M.OK, M.ARG]
    # rule 4: the random resource is the only worked group
    got = X.transcode(*args, first, off, lens, crc, nbt, 4, 0, sum(lens))
    assert list(got[4]) == [M.OK, M.ARG, M.ARG] and list(got[1]) == [0, 2, 2, 2] and got[5] == (2, 0, 0)
    # rule 6
    full = X.transcode(*args, first, off, lens, crc, nbt, 4, 1, sum(lens))
    got = X.transcode(*args, first, off, lens, crc, nbt, 4, 1, int(full[2][4]) - 1)
    assert list(full[4]) == [M.OK] * 3 and list(got[4]) == [M.OK, M.OK, M.BUF] and list(got[2]) == list(full[2])
    assert got[0] == full[0][: int(full[2][3])]
