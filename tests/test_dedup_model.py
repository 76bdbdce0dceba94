"""CPU: the dedup model (tests/dedup_model.py). The GPU tests compare mscomp_amd_deduper_dedup with this model entry for entry, so the model
is pinned here on hand-made containers (every block stored raw: the stored form is the data) and on containers the container model
compressed: by the header's consequence -- the picks spliced by tests/splice_model.py give a container whose resource new_index[g] is g --,
by the rules a refused resource falls under, and by the two collision constructions, where the count of the refuted is known."""
import zlib

import numpy as np
import pytest

import blocks_model as M
import dedup_model as D
import read_model as R
import splice_model as S
from dedup_model import raw_source, expect_two_orders
from splice_model import ORDER2, source

EMPTY, EMPTY_AGAIN, MIXED = D.EMPTY, 11, 5                      # rows of R.RECIPES


@pytest.fixture(scope="module")
def api():
    import ms_compress_amd                                       # noqa: F401  the model describes this library's deduper: no library, no test
    from ms_compress_amd import api
    assert "mscomp_amd_deduper_dedup" in api.EXPORTS
    return api


def spliced(sources, d, B, with_crc):
    """the picks of a dedup result, padding included, spliced by the splice model into a table with room for everything"""
    picks = [(d["pick"][2 * p], d["pick"][2 * p + 1]) for p in range(len(d["pick"]) // 2)]
    return S.model_splice(sources, picks, B, sum(int(s[7]) for s in sources), 1 << 40, with_crc=with_crc)


@pytest.mark.parametrize("with_crc", (True, False))
def test_two_orders_raw(api, with_crc):
    B = 4096
    bufs = R.buffers(B)
    n = len(bufs)
    sources = [raw_source(bufs, B), raw_source([bufs[k] for k in ORDER2], B)]
    d = D.model_dedup(sources, B, with_crc, n_res_total=2 * n + 3)
    assert d["status"] == [0] * (2 * n) and d["rep"] == expect_two_orders(n)
    assert d["rep"][EMPTY_AGAIN] == EMPTY                          # empties are equal, whatever their recipes
    uniq = [(0, r) for r in range(n - 1)]
    assert d["pick"][: 2 * (n - 1)] == [x for p in uniq for x in p] and d["pick"][2 * (n - 1):] == [D.PAD] * (2 * (n + 4)) and len(d["pick"]) == 2 * (2 * n + 3)
    assert d["new_index"] == d["rep"]                              # (the unique ones are 0 .. n - 2: rank and index agree)
    stored = sum(len(b) for b in bufs)
    assert d["count"] == [n - 1, 2 * n, stored, 0]
    new = spliced(sources, d, B, with_crc)
    assert new["status"] == [0] * (n - 1) + [M.ARG] * (n + 4)      # a padding pick is an empty resource, refused by splice's rule 1
    D.holds_consequence(sources, B, with_crc, d, new)


@pytest.mark.parametrize("B", (4096, 65536))
@pytest.mark.parametrize("fmt", ("lznt1", "xpress", "xpress_huff"))
def test_two_orders_compressed(api, oracle, fmt, B):
    f = {"lznt1": 2, "xpress": 3, "xpress_huff": 4}[fmt]
    bufs0, src0 = source(oracle, f, B)
    bufs1, src1 = source(oracle, f, B, ORDER2)
    n = len(bufs0)
    for sources, want in (([src0, src1], expect_two_orders(n)), ([src1], [0, 1, 2, 3, 4, 1] + list(range(6, n)))):
        for with_crc in (True, False):
            d = D.model_dedup(sources, B, with_crc)
            assert d["rep"] == want and d["count"][0] == n - 1 and d["count"][3] == 0 and len(d["pick"]) == 2 * len(want)
            D.holds_consequence(sources, B, with_crc, d, spliced(sources, d, B, with_crc))


def test_a_refused_resource_represents_nobody(api):
    B = 4096
    bufs = R.buffers(B)
    n = len(bufs)
    good = raw_source(bufs, B)
    packed, plen, first, off, lens, crc, _, nbt = good
    falling = first.copy(); falling[3] = falling[4] + np.uint64(1)         # resource 3 by rule 1, resource 2 by rule 2 (one row too many)
    beyond = first.copy(); beyond[n] = np.uint64(nbt + 1)                  # the last, empty resource by rule 1
    odd = list(lens); odd[MIXED] += B                                      # rule 2
    j = int(first[MIXED])
    past = off.copy(); past[j + 2:] = np.uint64(plen + 1)                  # rule 3 for MIXED (its row 1 ends beyond packed_len) and everything behind it
    back = off.copy(); back[j + 2] = back[j + 1] - np.uint64(1)            # rule 3 for MIXED alone: a decreasing entry, rows 1 and 2
    cases = ((good[:2] + (falling,) + good[3:], {3: M.ARG, 2: M.DATA}), (good[:2] + (beyond,) + good[3:], {n - 1: M.ARG}),
             (good[:4] + (odd,) + good[5:], {MIXED: M.DATA}), (good[:3] + (past,) + good[4:], {r: M.DATA for r in range(MIXED, n) if lens[r]}),
             (good[:3] + (back,) + good[4:], {MIXED: M.DATA}))
    for hurt, bad in cases:
        sources = [hurt, good]
        d = D.model_dedup(sources, B, True)
        for r in range(n):
            twin = n + r
            assert d["status"][r] == bad.get(r, 0) and d["status"][twin] == 0
            if r in bad:                                            # its own representative, picked; the healthy twin does not point at it
                assert d["rep"][r] == r and d["rep"][twin] != r and (0, r) in zip(d["pick"][0::2], d["pick"][1::2])
            elif lens[r]:
                assert d["rep"][r] == r and d["rep"][twin] == r
        empties = [g for g in (EMPTY, EMPTY_AGAIN, n + EMPTY, n + EMPTY_AGAIN) if d["status"][g] == 0]
        assert all(d["rep"][g] == empties[0] for g in empties)
        assert d["count"][0] == len(set(d["rep"])) and d["count"][3] == 0
        D.holds_consequence(sources, B, True, d, spliced(sources, d, B, True))


@pytest.mark.parametrize("B", (4096, 65536))
def test_full_key_collision_with_checksums(api, B):
    """a raw resource and its twin with the CRC polynomial XORed into the middle of block 1: equal lengths, equal CRC words, equal first and
    last 16 bytes of every row -- one key tuple, and only the byte compare tells them apart"""
    base = M.build({"kind": "random", "seed": 9, "mult": 3, "add": 17}, B)
    twin = D.crc_twin(base, B + B // 2)
    for ln in (5, 4096, 70000):                                    # the construction itself: the five bytes keep zlib's crc32 at any length
        blob = np.random.RandomState(ln).bytes(ln)
        assert zlib.crc32(D.crc_twin(blob, ln // 3 if ln > 5 else 0)) == zlib.crc32(blob)
    assert twin != base and zlib.crc32(twin) == zlib.crc32(base) and zlib.crc32(twin[B: 2 * B]) == zlib.crc32(base[B: 2 * B])
    sources = [raw_source([base, bytes(7)], B), raw_source([twin, base], B)]
    assert (sources[0][5][:4] == sources[1][5][:4]).all()
    d = D.model_dedup(sources, B, True)
    assert d["rep"] == [0, 1, 2, 0] and d["count"][0] == 3 and d["count"][3] == 1 and d["new_index"] == [0, 1, 2, 0]
    D.holds_consequence(sources, B, True, d, spliced(sources, d, B, True))
    d = D.model_dedup(sources, B, False)                           # without checksums the tuple is the same still
    assert d["rep"] == [0, 1, 2, 0] and d["count"][3] == 1


@pytest.mark.parametrize("B", (4096, 65536))
def test_several_classes_under_one_key(api, B):
    """A B C A B C of one length, the first and last 16 bytes of every block forced equal, no checksums: one key, three classes"""
    a, b, c = D.same_ends([M.build({"kind": "random", "seed": 40 + k, "mult": 2, "add": 100}, B) for k in range(3)], B)
    assert len({a, b, c}) == 3
    sources = [raw_source([a, b, c], B), raw_source([a, b, c], B)]
    d = D.model_dedup([(s[:5] + (None,) + s[6:]) for s in sources], B, False)
    assert d["rep"] == [0, 1, 2, 0, 1, 2] and d["count"] == [3, 6, 3 * len(a), 4] and d["new_index"] == [0, 1, 2, 0, 1, 2]
    d = D.model_dedup(sources, B, True)                            # with checksums the CRC words tell the keys apart
    assert d["rep"] == [0, 1, 2, 0, 1, 2] and d["count"][3] == 0
    D.holds_consequence(sources, B, True, d, spliced(sources, d, B, True))


def test_a_row_longer_than_a_block(api):
    """rules 1-3 bound a stored length by packed_len alone: one row of 5 B stored bytes under a resource of B bytes is accepted, and compared whole"""
    B = 4096
    data = M.build({"kind": "random", "seed": 31, "mult": 5, "add": 0}, B)
    other = bytearray(data); other[4 * B + 100] ^= 0x10

    def one_row(buf):
        s = raw_source([bytes(buf)], B)
        return (s[0], s[1], np.array([0, 1], dtype=np.uint64), np.array([0] + [5 * B] * s[7], dtype=np.uint64), [B], s[5], 1, s[7])
    for sources, rep, refuted in (([one_row(data), one_row(other)], [0, 1], 1), ([one_row(data), one_row(data)], [0, 0], 0)):
        d = D.model_dedup(sources, B, True)
        assert d["status"] == [0, 0] and d["rep"] == rep and d["count"][3] == refuted and d["count"][2] == (0 if refuted else 5 * B)
        D.holds_consequence(sources, B, True, d, spliced(sources, d, B, True))
