"""CPU: the diff model (tests/diff_model.py). The GPU tests compare mscomp_amd_deduper_diff with this model array for array, so the model is
pinned here on hand-made containers (every block stored raw: the stored form is the data) and on containers the container model compressed:
by the header's consequence -- the delta lists spliced out of the new container and the patch lists spliced over base and delta, both by
tests/extents_model.py, give the new container back --, by the bounds of the runs and the extents, by the rules a refused pair falls
under, and by the collision construction, where the count of the refuted is known."""
import numpy as np
import pytest

import blocks_model as M
import dedup_model as D
import diff_model as F
import read_model as R
from dedup_model import raw_source
from extents_model import source

NO = F.NO_BASE


@pytest.fixture(scope="module")
def api():
    import ms_compress_amd                                       # noqa: F401  the model describes this library's diff: no library, no test
    from ms_compress_amd import api
    assert "mscomp_amd_deduper_diff" in api.EXPORTS and api.MSCOMP_AMD_DIFF_NO_BASE == NO
    return api


def rand(seed, n):
    return np.random.RandomState(seed).bytes(n)


def poke(buf, at):
    out = bytearray(buf); out[at] ^= 0x5A
    return bytes(out)


def versions(B):
    """(base buffers, new buffers, per new resource the blocks that changed): R.RECIPES and what a day did to them"""
    base = R.buffers(B)
    new = list(base)
    new[3] = poke(base[3], 7)                                    # one block: its only one
    new[5] = poke(poke(poke(base[5], 0), B + B // 2), 3 * B + 16)   # 3 B + 17: the first, a middle and the last, short block
    new[6] = base[6] + rand(1, 3 * B)                            # longer by three blocks
    new[9] = base[9][: 3 * B]                                    # shorter by two
    new[8] = base[8] + rand(2, B - 17)                           # the short last block filled up: same leading bytes, another data length
    new[4] = poke(base[4], B)                                    # B + 1: the one byte of the last block
    new.append(rand(3, 2 * B + 5))                               # a resource the base does not have
    want = {3: [0], 5: [0, 1, 3], 6: [5, 6, 7], 8: [3], 4: [1], len(base): [0, 1, 2]}
    return base, new, want


def check(base, new, pairs, B, with_crc=True, room=None):
    room = sum((int(L) + B - 1) // B for L in new[4]) if room is None else room
    d = F.model_diff(base, new, pairs, B, room, with_crc)
    n_pair = len(pairs)
    assert len(d["status"]) == len(d["changed"]) == n_pair and len(d["delta_first"]) == len(d["patch_first"]) == n_pair + 1
    assert d["delta_first"][-1] == len(d["delta_ext"]) <= d["count"][0] <= d["count"][1] <= room      # a run has at least one row
    assert d["patch_first"][-1] == len(d["patch_ext"]) <= d["count"][1] and d["count"][3] <= d["count"][0] == sum(d["changed"])
    assert all(c != F.M64 and c > 0 for _, _, _, c in d["delta_ext"] + d["patch_ext"])                  # explicit counts, no empty run
    for p in range(n_pair):                                      # runs alternate, and cover the pair's blocks in order
        ext = d["patch_ext"][d["patch_first"][p]: d["patch_first"][p + 1]]
        assert all(x[0] != y[0] for x, y in zip(ext, ext[1:]))
        if d["status"][p] == 0:
            assert sum(c for _, _, _, c in ext) == len(d["verdicts"][p])
    delta, built = F.holds_consequence(base, new, pairs, d, B, room, with_crc)
    return d, delta, built


@pytest.mark.parametrize("with_crc", (True, False))
@pytest.mark.parametrize("B", (4096, 65536))
def test_versions_raw(api, B, with_crc):
    bufs0, bufs1, want = versions(B)
    base, new = raw_source(bufs0, B), raw_source(bufs1, B, spare=0)
    pairs = F.default_pairs(base, new)
    assert pairs[-1] == (NO, len(bufs0)) and pairs[0] == (0, 0)
    d, delta, built = check(base, new, pairs, B, with_crc)
    assert d["status"] == [0] * len(pairs) and d["count"][3] == (0 if with_crc else 5)     # the five poked blocks: only a checksum tells them in the tables
    for p, v in enumerate(d["verdicts"]):
        assert [k for k, x in enumerate(v) if x] == want.get(p, []), p
    F.same_container(built, new, with_crc)
    assert d["patch_ext"][d["patch_first"][5]: d["patch_first"][6]] == [(1, 5, 0, 2), (0, 5, 2, 1), (1, 5, 2, 1)]
    assert d["delta_ext"][d["delta_first"][5]: d["delta_first"][6]] == [(0, 5, 0, 2), (0, 5, 3, 1)]
    assert d["patch_ext"][d["patch_first"][6]: d["patch_first"][7]] == [(0, 6, 0, 5), (1, 6, 0, 3)]
    assert d["patch_ext"][d["patch_first"][9]: d["patch_first"][10]] == [(0, 9, 0, 3)]             # the base's blocks at and behind n_b are dropped
    assert d["patch_ext"][-1] == (1, len(bufs0), 0, 3)                                             # no base: one changed run
    assert d["count"][2] == sum(min(B, len(bufs1[p]) - k * B) for p, ks in want.items() for k in ks)


def test_identical_and_alternating(api):
    B = 4096
    bufs = R.buffers(B)
    src = raw_source(bufs, B)
    d, delta, built = check(src, src, F.default_pairs(src, src), B)
    assert d["count"] == [0, sum((len(b) + B - 1) // B for b in bufs), 0, 0] and d["delta_ext"] == []
    assert d["patch_ext"] == [(0, r, 0, (len(b) + B - 1) // B) for r, b in enumerate(bufs) if b]   # one base run per non-empty pair
    F.same_container(built, src)
    long = rand(5, 9 * B + 3)
    alt = long
    for k in range(0, 10, 2):
        alt = poke(alt, k * B + 1)
    base, new = raw_source([long], B), raw_source([alt], B)
    d, delta, built = check(base, new, [(0, 0)], B)
    assert d["count"][0] == 5 and len(d["patch_ext"]) == 10 == d["count"][1] and len(d["delta_ext"]) == 5      # the extent-count maximum
    assert d["patch_ext"][:3] == [(1, 0, 0, 1), (0, 0, 1, 1), (1, 0, 1, 1)]
    F.same_container(built, new)


def test_pairs_may_cross_and_repeat(api):
    B = 4096
    bufs = R.buffers(B)
    base, new = raw_source(bufs, B), raw_source(bufs[::-1], B)
    n = len(bufs)
    pairs = [(n - 1 - b, b) for b in range(n)] + [(3, n - 1 - 8), (NO, 2), (8, n - 1 - 7)]          # 3, 8: random; 7: text of 3 B + 17
    d, _, _ = check(base, new, pairs, B, room=200)
    assert d["changed"][:n] == [0] * n and d["changed"][n:] == [4, 5, 4]
    assert d["patch_ext"][-1] == (1, n + 2, 0, 4)


@pytest.mark.parametrize("B", (4096, 65536))
@pytest.mark.parametrize("f", (2, 3, 4))
def test_versions_compressed(api, oracle, f, B):
    bufs0, bufs1, want = versions(B)
    base, new = source(oracle, f, B, bufs0), source(oracle, f, B, bufs1)
    pairs = F.default_pairs(base, new)
    for with_crc in (True, False):
        d, delta, built = check(base, new, pairs, B, with_crc)
        assert d["status"] == [0] * len(pairs) and (d["count"][3] == 0 or not with_crc)
        for p, v in enumerate(d["verdicts"]):
            assert [k for k, x in enumerate(v) if x] == want.get(p, []), p
        F.same_container(built, new, with_crc)


@pytest.mark.parametrize("with_crc", (True, False))
def test_refuted_is_exact(api, with_crc):
    """a raw block and its twin with the CRC polynomial XORed into its middle: equal lengths, equal CRC words, other bytes"""
    B = 4096
    data = rand(11, 3 * B + 100)
    twin = D.crc_twin(data, B + B // 2)
    base, new = raw_source([data, data], B), raw_source([twin, data], B)
    assert (base[5] == new[5]).all()
    d, _, built = check(base, new, [(0, 0), (1, 1)], B, with_crc)
    assert d["count"] == [1, 8, B, 1] and d["changed"] == [1, 0] and d["patch_ext"][:3] == [(0, 0, 0, 1), (1, 0, 0, 1), (0, 0, 2, 2)]
    F.same_container(built, new, with_crc)
    far = raw_source([poke(data, 2 * B + 2000), data], B)          # a plain change: refuted only when no checksum tells
    d, _, _ = check(base, far, [(0, 0), (1, 1)], B, with_crc)
    assert d["count"][0] == 1 and d["count"][3] == (0 if with_crc else 1)


def test_refusals(api):
    B = 4096
    bufs = R.buffers(B)
    n = len(bufs)
    good = raw_source(bufs, B)
    packed, plen, first, off, lens, crc, _, nbt = good
    MIXED = 5
    falling = first.copy(); falling[3] = falling[4] + np.uint64(1)         # resource 3 by dedup's rule 1, resource 2 by its rule 2
    odd = list(lens); odd[MIXED] += B                                      # dedup's rule 2
    j = int(first[MIXED])
    back = off.copy(); back[j + 2] = back[j + 1] - np.uint64(1)            # dedup's rule 3 for MIXED: rows 1 and 2
    hurt = {"falling": (good[:2] + (falling,) + good[3:], {3: M.ARG, 2: M.DATA}), "odd": (good[:4] + (odd,) + good[5:], {MIXED: M.DATA}),
            "back": (good[:3] + (back,) + good[4:], {MIXED: M.DATA})}
    pairs = [(r, r) for r in range(n)]
    for name, (src, bad) in hurt.items():
        for base, new in ((src, good), (good, src)):                       # either side
            d, _, _ = check(base, new, pairs, B)
            assert d["status"] == [bad.get(r, 0) for r in range(n)], name
            assert all(d["changed"][r] == 0 for r in range(n)), name       # the neighbours of a refused pair: untouched, and in place
            assert [e[1] for e in d["patch_ext"]] == [r for r in range(n) if lens[r] and r not in bad], name
    # rule 1, and the order of the rules: the indices before any table, dedup's rule 1 on either side before its rule 2 on either
    both = (hurt["falling"][0], hurt["odd"][0])
    d, _, _ = check(both[0], both[1], [(0, n), (n, 0), (NO, n), (NO, 1), (2, MIXED), (MIXED, 3), (3, MIXED), (MIXED, MIXED)], B, room=64)
    assert d["status"] == [M.ARG, M.ARG, M.ARG, 0, M.DATA, 0, M.ARG, M.DATA]
    # a base row behind n_b is dropped, not judged
    cut = raw_source([bufs[MIXED][:B]], B)
    d, _, _ = check(hurt["back"][0], cut, [(MIXED, 0)], B)
    assert d["status"] == [0] and d["changed"] == [0] and d["patch_ext"] == [(0, MIXED, 0, 1)]
    # rule 3: room exhausted at a middle pair; pairs without blocks pass behind it
    d, _, _ = check(good, good, pairs, B, room=6)
    used = np.cumsum([(x + B - 1) // B for x in lens])
    assert d["status"] == [0 if (u <= 6 or not x) else M.ARG for u, x in zip(used, lens)] and M.ARG in d["status"][1: n - 1] and d["status"][n - 1] == 0
    assert d["count"][1] == 5


def test_no_pairs(api):
    B = 4096
    src = raw_source(R.buffers(B), B)
    d = F.model_diff(src, src, [], B, 0)
    assert d["count"] == [0, 0, 0, 0] and d["delta_first"] == [0] and d["patch_first"] == [0]
