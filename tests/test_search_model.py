"""CPU: tests/search_model.py against a comparison at every position, byte by byte, on small seeded data, and the corners of the contract
(search_model.EDGES) asserted to be reached by the calls the GPU tests make the same way."""
import numpy as np
import pytest

import blocks_model as M
import search_model as S

B = 4096
FMT = 3                                                            # Xpress: the container's codec does not matter to the rules


@pytest.fixture(scope="module")
def container(oracle):
    bufs = S.buffers(B)
    total = sum(len(b) for b in bufs)
    packed, first, off, st = M.model_compress(oracle, FMT, bufs, B, total, total)
    assert not st.any()
    stored = np.diff(off[: int(first[-1]) + 1].astype(np.int64))
    assert (stored == B).any() and (stored < 64).any()            # raw and compressed blocks
    return bufs, packed, first, off


def run(oracle, container, reqs, pats, len_max=None, blocks_max=10 ** 6, hits_max=10 ** 6, blob_off=None):
    bufs, packed, first, off = container
    blob, poff = blob_off or S.pack_patterns(pats)
    len_max = len_max or max(1, min(256, max(len(p) for p in pats)))
    return S.model_search(oracle, FMT, packed, len(packed), first, off, [len(b) for b in bufs], B, len(off) - 1, reqs, blob, poff, len_max, blocks_max, hits_max)


def as_triples(mo):
    return [(w >> 32, x, w & 0xFFFFFFFF) for x, w in mo["records"]]


def test_the_model_is_the_comparison_at_every_position(oracle, container):
    bufs = container[0]
    rs = np.random.RandomState(5)
    pats = [b"\x01", b"\x02\x03", b"\x07\x00\x01", b"\x01\x01\x01\x01", b"\x03\x02\x01\x00\x05", S.NEEDLE, S.NEEDLE, b"a", b"aa", b"aaaa", S.END1, S.END3,
            S.END3[1:], S.END3[2:], S.END1 + S.END3[:1], bufs[S.MIX][2 * B - 100: 2 * B + 156], bufs[S.MIX][B - 3: B + 6]]
    reqs = [(r, 0, M.M64) for r in range(len(bufs))]
    for _ in range(24):                                            # ranges that start and end anywhere, some behind the end
        r = int(rs.randint(0, len(bufs)))
        reqs.append((r, int(rs.randint(0, len(bufs[r]) + 3)), int(rs.randint(0, 2 * B))))
    mo = run(oracle, container, reqs, pats)
    want = S.brute(bufs, reqs, pats, 256)
    assert as_triples(mo) == want and mo["count"] == [len(want), len(want)]
    assert mo["req_hits"] == [sum(1 for t in want if t[0] == q) for q in range(len(reqs))]
    assert mo["status"] == [0] * len(reqs) and mo["pat_status"] == [0] * len(pats)
    # the first hits_max of the same order
    cut = run(oracle, container, reqs, pats, hits_max=1000)
    assert as_triples(cut) == want[:1000] and cut["count"] == [len(want), 1000] and cut["req_hits"] == mo["req_hits"]


def test_find_all_counts_overlapping_occurrences():
    assert S.find_all(b"aaaaa", b"aa", 0, 5) == [0, 1, 2, 3] and S.find_all(b"aaaaa", b"aa", 1, 3) == [1, 2] and S.find_all(b"abcabc", b"bc", 0, 4) == [1]
    assert S.find_all(b"abc", b"abcd", 0, 3) == []


def test_every_edge_is_reached(oracle, container):
    bufs = container[0]
    L6, reached = len(bufs[S.SOFT_FIRST]), set()
    # patterns: the needle twice, three refused ones (empty, backwards, too long), the ends
    blob = S.NEEDLE + S.NEEDLE + S.END3[1:] + S.END1 + S.END3[:1] + bytes(300)
    poff = [0, 5, 10, 10, 12, 10, 12, 14, 14 + 257]                # needle, needle, empty, END3[1:], backwards, END3[1:], END1 + END3[0], 257 zeros
    reqs = [(S.SOFT_FIRST, 0, M.M64), (S.RANDOM_FIRST, 0, M.M64), (S.THREE, 0, M.M64), (S.ONE, 0, M.M64), (S.B_MORE, 0, M.M64), (len(bufs), 0, 1),
            (S.SOFT_FIRST, 0, B - 1), (S.SOFT_FIRST, B - 1, B - 1), (S.SOFT_FIRST, 0, 3 * B - 3)]
    mo = run(oracle, container, reqs, None, len_max=256, blob_off=(blob, poff))
    reached |= mo["edges"]
    assert mo["pat_status"] == [0, 0, M.ARG, 0, M.ARG, 0, 0, M.ARG] and mo["status"] == [0] * 5 + [M.ARG] + [0] * 3
    hits = as_triples(mo)
    assert [x for q, x, p in hits if q == 0 and p == 0] == [0, B - 1, 2 * B - 2, 3 * B - 3, 4 * B - 4, 5 * B - 5, L6 - 5]
    assert [(x, p) for q, x, p in hits if q == 2] == [(1, 3), (1, 5)] and not [t for t in hits if t[2] == 6]      # nothing spans two resources
    assert [x for q, x, p in hits if q == 6 and p == 0] == [0]                                                # the needle at B - 1 starts at the range's end
    assert [x for q, x, p in hits if q == 7 and p == 0] == [B - 1] and [x for q, x, p in hits if q == 8 and p == 0] == [0, B - 1, 2 * B - 2]
    # the run: dense overlapping hits, and more of them than there is room for
    mo = run(oracle, container, [(S.RUN, 0, M.M64)], [b"a", b"aa", b"aaaa"], hits_max=100)
    reached |= mo["edges"]
    assert mo["count"] == [3 * 3 * B - 1 - 3, 100] and as_triples(mo)[:5] == [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 1, 0), (0, 1, 1)]
    # the budget: the look-ahead's block alone goes over it
    mo = run(oracle, container, [(S.SOFT_FIRST, 0, B), (S.SOFT_FIRST, 0, B)], [S.NEEDLE], blocks_max=3)
    reached |= mo["edges"]
    assert mo["status"] == [0, M.ARG] and mo["req_hits"] == [2, 0]           # (the one at B - 1 with its tail in the look-ahead)
    # a pattern cut by the resource's end: the last four bytes of the needle at the end of B_MORE are there, its fifth is not
    mo = run(oracle, container, [(S.B_MORE, 0, M.M64)], [S.NEEDLE[1:] + b"\x00"])
    reached |= mo["edges"]
    assert mo["count"] == [0, 0]
    assert reached == set(S.EDGES), sorted(set(S.EDGES) - reached)
