"""CPU: the match model (tests/match_model.py). The GPU tests compare mscomp_amd_deduper_match with this model array for array, so the model
is pinned here on hand-made containers (every block stored raw: the stored form is the data) and on containers the container model
compressed: by the header's consequence -- the delta lists spliced out of the new container and the patch lists spliced over the stores
and the delta, both by tests/extents_model.py, give the new container back --, by the bounds of the runs and the extents, by the rules a
refused resource falls under, by the collision construction, where the count of the refuted is known, and by one cross-check against
tests/diff_model.py."""
import numpy as np
import pytest

import blocks_model as M
import dedup_model as D
import diff_model as F
import match_model as T
import read_model as R
from dedup_model import raw_source
from extents_model import source

FOUND, SHARED, FRESH = T.FOUND, T.SHARED, T.FRESH


@pytest.fixture(scope="module")
def api():
    import ms_compress_amd                                       # noqa: F401  the model describes this library's match: no library, no test
    from ms_compress_amd import api
    assert "mscomp_amd_deduper_match" in api.EXPORTS and "mscomp_amd_deduper_create_match" in api.EXPORTS
    return api


def rand(seed, n):
    return np.random.RandomState(seed).bytes(n)


def blocks_of(src, B):
    return sum((int(L) + B - 1) // B for L in src[4])


def check(stores, new, B, with_crc=True, total=None, room=None):
    room = blocks_of(new, B) if room is None else room
    total = sum(blocks_of(s, B) for s in stores) + room if total is None else total
    d = T.model_match(stores, new, B, total, room, with_crc)
    n_new = int(new[6])
    assert len(d["status"]) == sum(int(s[6]) for s in stores) + n_new and len(d["cls"]) == 3 * n_new
    assert len(d["delta_first"]) == len(d["patch_first"]) == n_new + 1
    assert d["delta_first"][-1] == len(d["delta_ext"]) <= d["count"][2] <= d["count"][3] <= room            # a run has at least one row
    assert d["patch_first"][-1] == len(d["patch_ext"]) <= d["count"][3] == d["count"][0] + d["count"][1] + d["count"][2]
    assert [sum(d["cls"][i::3]) for i in range(3)] == d["count"][:3]
    assert all(c != T.M64 and c > 0 for _, _, _, c in d["delta_ext"] + d["patch_ext"])                       # explicit counts, no empty run
    for q in range(n_new):                                         # the runs cover the resource's blocks in order
        ext = d["patch_ext"][d["patch_first"][q]: d["patch_first"][q + 1]]
        if d["status"][d["n_store"] + q] == 0:
            assert sum(c for _, _, _, c in ext) == len(d["classes"][q])
        else:
            assert ext == [] and d["classes"][q] is None
    delta, built = T.holds_consequence(stores, new, d, B, room, with_crc)
    return d, delta, built


@pytest.mark.parametrize("with_crc", (True, False))
@pytest.mark.parametrize("B", (4096, 65536))
def test_moves_raw(api, B, with_crc):
    """every block of the store is somewhere else in the new container; one block is new"""
    a, b, c = rand(1, 3 * B + 17), rand(2, 2 * B), rand(3, B + 1)
    extra = rand(4, B)
    store = raw_source([a, b, c, b""], B)
    new = raw_source([c, extra + a, b"", b + a[: 2 * B], b[B:] + b[:B]], B, spare=0)
    d, delta, built = check([store], new, B, with_crc)
    assert d["status"] == [0] * 9 and d["count"][:4] == [12, 0, 1, 13] and d["count"][4] == B and d["count"][5] == 0
    assert d["patch_ext"] == [(0, 2, 0, 2),                                       # a permuted resource: one run
                              (1, 1, 0, 1), (0, 0, 0, 4),                         # a block inserted at the front: everything behind it ONE run, short tail included
                              (0, 1, 0, 2), (0, 0, 0, 2),                         # a concatenation at a block boundary: one run per part
                              (0, 1, 1, 1), (0, 1, 0, 1)]                         # two blocks swapped: two runs
    assert d["delta_ext"] == [(0, 1, 0, 1)] and d["cls"] == [2, 0, 0, 4, 0, 1, 0, 0, 0, 4, 0, 0, 2, 0, 0]
    F.same_container(built, new, with_crc)
    d, delta, built = check([store], store, B, with_crc)                            # identity: all found, D has no rows
    assert d["count"][:5] == [8, 0, 0, 8, 0] and d["delta_ext"] == [] and len(delta["packed"]) == 0
    assert d["patch_ext"] == [(0, 0, 0, 4), (0, 1, 0, 2), (0, 2, 0, 2)]
    F.same_container(built, store, with_crc)


def test_sharing_and_single_instance(api):
    B = 4096
    x, y, z = rand(5, B), rand(6, B), rand(7, B)
    new = raw_source([x + y + x, z + x, x + y, y + x], B, spare=0)
    d, delta, built = check([], new, B)                                              # no store: the container against itself
    assert d["classes"] == [[FRESH, FRESH, SHARED], [FRESH, SHARED], [SHARED, SHARED], [SHARED, SHARED]]
    assert d["patch_ext"] == [(0, 0, 0, 2), (0, 0, 0, 1), (0, 1, 0, 1), (0, 0, 0, 1),
                              (0, 0, 0, 2),                                       # representatives consecutive: one run
                              (0, 0, 1, 1), (0, 0, 0, 1)]                         # the same two, swapped: two runs
    assert d["count"] == [0, 6, 3, 9, 3 * B, 0] and len(delta["packed"]) == 3 * B
    F.same_container(built, new)
    zeros = raw_source([bytes(5 * B)], B, spare=0)                                   # the smallest equal row always wins: one extent per block
    d, _, built = check([], zeros, B)
    assert d["patch_ext"] == [(0, 0, 0, 1)] * 5 and d["count"][:3] == [0, 4, 1]
    F.same_container(built, zeros)


def test_smallest_wins_and_short_blocks(api):
    B = 4096
    x, t = rand(8, B), rand(9, 100)
    s0, s1 = raw_source([rand(10, B), x + t], B), raw_source([x, x + t, x[:100]], B)
    new = raw_source([x + t, t, x[:100], x[:50]], B, spare=0)
    d, _, built = check([s0, s1], new, B)
    # x is found in the first store that has it, and the short tail t only as a short block of ITS data length; x[:100] is the head of a full block and
    # of t's length, and neither makes it found anywhere but at its own copy; x[:50] is fresh
    assert d["patch_ext"] == [(0, 1, 0, 2), (0, 1, 1, 1), (1, 2, 0, 1), (2, 3, 0, 1)] and d["count"][:3] == [4, 0, 1]
    F.same_container(built, new)
    twice = raw_source([t, t, x + t], B, spare=0)                                    # equal tails are shared too
    d, _, built = check([], twice, B)
    assert d["classes"] == [[FRESH], [SHARED], [FRESH, SHARED]] and d["patch_ext"][-1] == (0, 0, 0, 1)
    F.same_container(built, twice)
    # stored bytes agree, data lengths differ (an edited length table): the data-length clause decides
    a, other = raw_source([x + t], B, spare=0), raw_source([t], B, spare=0)
    d, _, _ = check([a], other, B)
    assert d["count"][:3] == [1, 0, 0]
    fat = other[:4] + ([200],) + other[5:]                                        # the same 100 stored bytes as a block of 200 data bytes
    d, _, _ = check([a], fat, B)
    assert d["count"][:3] == [0, 0, 1] and d["count"][5] == 0                      # another tuple: not even a candidate


@pytest.mark.parametrize("with_crc", (True, False))
def test_refuted_chain(api, with_crc):
    """raw blocks that agree in length and in their first and last 16 bytes and differ in the middle"""
    B = 4096
    x1, x2, x3 = D.same_ends([rand(21, B), rand(22, B), rand(23, B)], B)
    store, new = raw_source([x1 + x2], B), raw_source([x2 + x3 + x3], B, spare=0)
    if with_crc:                                                   # checksums that agree, by an edit of the tables
        same = lambda s: s[:5] + (np.full(len(s[5]), 0x1234, dtype=np.uint32),) + s[6:]
        store, new = same(store), same(new)
    d, _, built = check([store], new, B, with_crc)
    assert d["patch_ext"] == [(0, 0, 1, 1), (1, 0, 0, 1), (1, 0, 0, 1)]              # x2 at x2's row, not x1's; x3 fresh, then shared
    assert d["classes"] == [[FOUND, FRESH, SHARED]] and d["count"] == [1, 1, 1, 3, B, 4]
    F.same_container(built, new, with_crc)
    if not with_crc:                                               # with honest checksums the tuples differ: nothing is refuted
        d, _, _ = check([raw_source([x1 + x2], B)], raw_source([x2 + x3 + x3], B, spare=0), B, True)
        assert d["count"] == [1, 1, 1, 3, B, 0]


@pytest.mark.parametrize("B", (4096, 65536))
@pytest.mark.parametrize("f", (2, 3, 4))
def test_moves_compressed(api, oracle, f, B):
    bufs = R.buffers(B)
    store = source(oracle, f, B, bufs)
    moved = [bufs[k] for k in (9, 0, 5, 3, 11, 1)] + [rand(31, B) + bufs[7], bufs[8][: 2 * B] + bufs[4]]   # (7: text of 3 B + 17)
    new = source(oracle, f, B, moved)
    for with_crc in (True, False):
        d, delta, built = check([store], new, B, with_crc)
        assert all(s == 0 for s in d["status"]) and d["count"][5] == 0
        assert d["cls"][3 * 6: 3 * 6 + 3][2] == 1 and d["count"][2] == 1           # the one inserted block is all that is fresh ...
        assert d["patch_ext"][d["patch_first"][6]: d["patch_first"][7]][1][3] == 4  # ... and the four blocks behind it are one run
        F.same_container(built, new, with_crc)


def test_refusals_and_room(api):
    B = 4096
    bufs = [rand(41, 2 * B), rand(42, 3 * B + 17), rand(43, B), b""]
    good = raw_source(bufs, B)
    packed, plen, first, off, lens, crc, n, nbt = good
    falling = first.copy(); falling[1] = falling[2] + np.uint64(1)          # resource 1 by rule 1, resource 0 by rule 2
    odd = list(lens); odd[1] += B                                          # rule 2
    back = off.copy(); back[4] = back[3] - np.uint64(1)                    # rule 3 for resource 1: rows 2 .. 5
    hurt = {"falling": (good[:2] + (falling,) + good[3:], {1: M.ARG, 0: M.DATA}), "odd": (good[:4] + (odd,) + good[5:], {1: M.DATA}),
            "back": (good[:3] + (back,) + good[4:], {1: M.DATA})}
    for name, (src, bad) in hurt.items():
        d, _, _ = check([src], good, B)                                    # a refused store resource brings no rows: its blocks are fresh
        assert d["status"] == [bad.get(r, 0) for r in range(n)] + [0] * n, name
        assert d["cls"] == [x for r in range(n) for x in ((0, 0, (lens[r] + B - 1) // B) if r in bad else ((lens[r] + B - 1) // B, 0, 0))], name
        d, _, _ = check([good], src, B)                                    # a refused resource of new: no extents, zero counts, indices in place
        assert d["status"] == [0] * n + [bad.get(r, 0) for r in range(n)], name
        assert [e[1] for e in d["patch_ext"]] == [r for r in range(n) if lens[r] and r not in bad], name
        assert d["count"][1:3] == [0, 0], name
    # rule 4: at exactly the bound everything passes; one below, the resource that crosses it is refused, the empty one behind it is not
    rows = blocks_of(good, B)
    d, _, _ = check([good], good, B, total=2 * rows, room=rows)
    assert d["status"] == [0] * 8
    d, _, _ = check([good], good, B, total=2 * rows, room=rows - 1)
    assert d["status"] == [0] * 4 + [0, 0, M.ARG, 0] and d["count"][3] == 6
    d, _, _ = check([good], good, B, total=2 * rows - 1, room=rows)          # the total over all rows
    assert d["status"] == [0] * 4 + [0, 0, M.ARG, 0]
    d, _, _ = check([good], good, B, total=3, room=rows)                     # refused in a store: counted, and everything behind it with rows too
    assert d["status"] == [0, M.ARG, M.ARG, 0, M.ARG, M.ARG, M.ARG, 0] and d["count"][:4] == [0, 0, 0, 0]


def test_against_diff(api):
    """where no two blocks of store and new are equal except at the same (resource, index), the fresh set is diff's changed set"""
    B = 4096
    base_bufs = [rand(51, 3 * B + 17), rand(52, 2 * B), rand(53, B + 1)]
    poke = lambda buf, at: buf[:at] + bytes([buf[at] ^ 0x5A]) + buf[at + 1:]
    new_bufs = [poke(poke(base_bufs[0], 5), 3 * B + 3), base_bufs[1] + rand(54, B), poke(base_bufs[2], B)]
    base, new = raw_source(base_bufs, B), raw_source(new_bufs, B, spare=0)
    for with_crc in (True, False):
        d, _, _ = check([base], new, B, with_crc)
        f = F.model_diff(base, new, F.default_pairs(base, new), B, blocks_of(new, B), with_crc)
        assert [[c == FRESH for c in kinds] for kinds in d["classes"]] == f["verdicts"]
        assert d["delta_ext"] == f["delta_ext"] and d["delta_first"] == f["delta_first"]
        assert [d["count"][2], d["count"][3], d["count"][4]] == f["count"][:3] and d["count"][1] == 0


def test_empty(api):
    B = 4096
    none = raw_source([], B, spare=0)
    d, _, _ = check([], none, B)
    assert d["count"] == [0] * 6 and d["delta_first"] == [0] and d["patch_first"] == [0]
    some = raw_source([rand(61, B + 5)], B)
    d, _, _ = check([some, none], none, B)
    assert d["count"] == [0] * 6 and d["status"] == [0]
