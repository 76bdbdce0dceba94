"""GPU: block searchers (mscomp_amd_searcher_*, include/mscomp_amd_search.h) against the model of tests/search_model.py on containers made by
BlockContainer.compress: the records word for word, d_req_hits, d_count, d_pat_status and d_status entry by entry, the reader's three
counts, and sentinels behind every array the call writes."""
import numpy as np
import pytest

import blocks_model as M
import search_model as S
from blocks_rig import Container, d64, flip, flipped, memo, FMTS, ALL, ENTRY_GUARD, SENT, SENT32

pytestmark = pytest.mark.gpu
B = 4096
GUARD = 2 * ENTRY_GUARD


class SearchRig(Container):
    """a container made on the GPU once; search() runs one call with sentinel-filled outputs, check() compares all of them with the model"""

    def search(self, reqs, blob, poff, len_max, blocks_max, hits_max, crc=False, first=None, boff=None, packed=None, packed_len=None, searcher=None):
        import torch
        dev, nq, npat = self.dev, len(reqs), len(poff) - 1
        sr = searcher or self.m.BlockSearcher(self.ctx, self.fmt, self.B, self.n, self.nbt, nq, blocks_max, npat, len_max, hits_max)
        full = lambda k, v, t: torch.full((k,), v, dtype=t, device=dev)
        d_req = d64(np.array(reqs, dtype=np.uint64), dev, 3)
        d_pat = torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()).to(dev)
        d_poff = d64(np.array([int(x) & ALL for x in poff], dtype=np.uint64), dev)
        d_hits, d_rh, d_cnt = full(2 * hits_max + GUARD, SENT, torch.int64), full(nq + GUARD, SENT, torch.int64), full(2 + GUARD, SENT, torch.int64)
        d_pst, d_st = full(npat + GUARD, SENT32, torch.int32), full(nq + GUARD, SENT32, torch.int32)
        sr.search(self.d_packed if packed is None else packed, self.plen if packed_len is None else packed_len,
                  self.d_first if first is None else d64(first, dev), self.d_boff if boff is None else d64(boff, dev), self.d_len,
                  self.d_crc if crc else None, d_req, d_pat, d_poff, d_hits, d_rh, d_cnt, d_pst, d_st)
        counts = sr.counts()
        if searcher is None:
            sr.close()
        u64 = lambda t: t.cpu().numpy().view(np.uint64)
        return {"hits": u64(d_hits), "req_hits": u64(d_rh), "count": u64(d_cnt), "pat_status": d_pst.cpu().numpy(), "status": d_st.cpu().numpy(), "counts": counts}

    def check(self, oracle, reqs, pats, len_max=None, blocks_max=None, hits_max=None, crc=False, model_packed=None, **kw):
        """``pats``: byte strings, or (blob, pat_off). Returns the model's answer."""
        blob, poff = pats if isinstance(pats, tuple) else S.pack_patterns(pats)
        len_max = len_max or max(1, min(S.LEN_MAX, max(b - a for a, b in zip(poff[:-1], poff[1:]))))
        budget = self.searched(reqs, len_max) if blocks_max is None else blocks_max
        model = lambda room: S.model_search(oracle, self.fmt, self.packed if model_packed is None else model_packed,
                                            self.plen if kw.get("packed_len") is None else kw["packed_len"],
                                            self.first if kw.get("first") is None else kw["first"], self.off if kw.get("boff") is None else kw["boff"],
                                            self.lens, self.B, self.nbt, reqs, blob, poff, len_max, budget, room, self.crc if crc else None)
        room = model(0)["count"][0] + 3 if hits_max is None else hits_max
        mo = model(room)
        got = self.search(reqs, blob, poff, len_max, budget, room, crc, **kw)
        same_words(got["status"], mo["status"], SENT32, "d_status")
        same_words(got["pat_status"], mo["pat_status"], SENT32, "d_pat_status")
        same_words(got["count"], mo["count"], SENT, "d_count")
        same_words(got["req_hits"], mo["req_hits"], SENT, "d_req_hits")
        same_words(got["hits"], [w for rec in mo["records"] for w in rec], SENT, "d_hits")
        assert got["counts"] == mo["counts"], ("counts", got["counts"], mo["counts"])
        return mo

    def searched(self, reqs, len_max):
        """the searcher's budget of the requests: their covering blocks with the look-ahead's"""
        out = 0
        for r, o, ln in reqs:
            if r < self.n:
                L = self.lens[r]
                o = min(o, L)
                w = min(ln, L - o)
                out += ((min(L, o + w + len_max - 1) - 1) // self.B - o // self.B + 1) if w else 0
        return out


def same_words(got, want, sentinel, what):
    """``got`` begins with ``want``, entry by entry, and holds nothing but its sentinel behind it"""
    want = np.asarray([int(x) for x in want], dtype=got.dtype)
    bad = np.nonzero(got[: len(want)] != want)[0]
    assert bad.size == 0, (what, "differs at entry", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
    assert (got[len(want):] == np.asarray(sentinel).astype(got.dtype)).all(), (what, "written behind the entries in use")


def triples(mo):
    return [(w >> 32, x, w & 0xFFFFFFFF) for x, w in mo["records"]]


def whole(rig):
    return [(r, 0, ALL) for r in range(rig.n)]


@pytest.fixture(scope="module")
def rigs(gpu_ctx):
    yield from memo(lambda fmt: SearchRig.make(gpu_ctx, FMTS[fmt], B, S.buffers(B)))


@pytest.mark.parametrize("fmt", list(FMTS))
def test_boundaries_ends_and_patterns(rigs, oracle, fmt):
    """every resource whole, against: the needle at every split across raw/decoded boundaries in both orders, twice; patterns of 1, 2 and 3
    bytes in the last bytes of a resource; one that would span two resources and one cut by a resource's end; a pattern of 256 bytes;
    three refused ones (empty, offsets backwards, 257 bytes at len_max 256)"""
    rig = rigs(fmt)
    stored = np.diff(rig.off[: int(rig.first[-1]) + 1].astype(np.int64))
    j7, j8 = int(rig.first[S.SOFT_FIRST]), int(rig.first[S.RANDOM_FIRST])
    assert [int(s) == B for s in stored[j7: j7 + 6]] == [False, True] * 3 and [int(s) == B for s in stored[j8: j8 + 6]] == [True, False] * 3
    long = rig.bufs[S.MIX][2 * B - 100: 2 * B + 156]
    blob = S.NEEDLE + S.NEEDLE + S.END3 + S.END1 + S.END3[:1] + S.NEEDLE[1:] + b"\x00" + long + bytes(300)
    at = 10 + 3 + 2 + 5                                            # where the 256 bytes begin
    # d_pat_off is one column, pattern p between entries p and p + 1: the needle, the needle, nothing, END3, END1
    mo = rig.check(oracle, whole(rig), (blob, [0, 5, 10, 10, 13, 14]), len_max=256, crc=True)
    assert mo["pat_status"] == [0, 0, M.ARG, 0, 0] and mo["status"] == [0] * rig.n and 0 < mo["counts"][2] < mo["counts"][1] == int(rig.first[-1])
    hits, L = triples(mo), 6 * B
    for p in (0, 1):
        for r in (S.SOFT_FIRST, S.RANDOM_FIRST):
            assert [x for q, x, pp in hits if q == r and pp == p] == [0, B - 1, 2 * B - 2, 3 * B - 3, 4 * B - 4, 5 * B - 5, L - 5]
        assert [x for q, x, pp in hits if q == S.B_MORE and pp == p] == [B - 4] and [x for q, x, pp in hits if q == S.MIX and pp == p] == [3 * B]
    assert [(q, x) for q, x, p in hits if p == 3] == [(S.THREE, 0)] and [(q, x) for q, x, p in hits if p == 4][0] == (S.ONE, 0)
    # backwards, END3[0], END3[1:], backwards, END3[2], END1 + END3[0] (adjacent in d_packed, in two resources), the needle's tail and a byte
    # (cut by the end of B_MORE), nothing, 256 bytes, 257 bytes, backwards, END1 + END3[0] again
    poff = [13, 10, 11, 13, 12, 13, 15, 20, at, at + 256, at + 256 + 257, 13, 15]
    mo = rig.check(oracle, whole(rig), (blob, poff), len_max=256)
    assert mo["pat_status"] == [M.ARG, 0, 0, M.ARG, 0, 0, 0, M.ARG, 0, M.ARG, M.ARG, 0]
    ends = [(q, x, p) for q, x, p in triples(mo) if q in (S.ONE, S.THREE, S.B_MORE) and p != 8]
    assert ends == [(S.THREE, 0, 1), (S.THREE, 1, 2), (S.THREE, 2, 4)]
    assert [(q, x) for q, x, p in triples(mo) if p == 8] == [(S.MIX, 2 * B - 100)]
    assert {"hit_spans_blocks", "filter_past_end", "pattern_refused_backwards", "pattern_refused_long", "pattern_refused_empty", "cut_by_resource_end"} <= mo["edges"]


@pytest.mark.parametrize("fmt", list(FMTS))
def test_dense_run_overflow_and_no_room(rigs, oracle, fmt):
    rig = rigs(fmt)
    pats, total = [b"a", b"aa", b"aaaa"], 9 * B - 4
    mo = rig.check(oracle, [(S.RUN, 0, ALL)], pats)
    assert mo["count"] == [total, total] and triples(mo)[:7] == [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 1, 0), (0, 1, 1), (0, 1, 2), (0, 2, 0)]
    assert triples(mo)[-4:] == [(0, 3 * B - 3, 1), (0, 3 * B - 2, 0), (0, 3 * B - 2, 1), (0, 3 * B - 1, 0)]
    for room in (total - 1, 3 * B + 1, 100, 1, 0):                  # the first hits_max records, the exact counts, the sentinels behind 2 hits_max words
        mo = rig.check(oracle, [(S.RUN, 0, ALL), (S.RUN, B - 2, 5)], pats, hits_max=room)
        assert mo["count"] == [total + 15, room] and mo["req_hits"] == [total, 15]


@pytest.mark.parametrize("fmt", list(FMTS))
def test_ranges_inside_blocks(rigs, oracle, fmt):
    rig = rigs(fmt)
    r = S.SOFT_FIRST
    # the needle at B - 1: found by the range whose last position it starts at, not by the one that ends in front of it
    reqs = [(r, 7, B - 7), (r, 7, B - 8), (r, B - 1, 1), (r, B, ALL), (r, 1, 2 * B - 3), (r, 2 * B - 2, 1)]
    mo = rig.check(oracle, reqs, [S.NEEDLE])
    assert mo["req_hits"] == [1, 0, 1, 5, 1, 1] and {"tail_outside_range", "start_at_range_end_not_found", "lookahead_block_only"} <= mo["edges"]
    # two ranges that tile a resource find every hit once, wherever the cut lies
    pats = [S.NEEDLE, b"\x01\x02", b"\x07", rig.bufs[r][B + 30: B + 39]]
    everything = triples(rig.check(oracle, [(r, 0, ALL)], pats))
    for cut in (1, B - 4, B - 1, B, B + 1, 2 * B - 2, 3 * B + 77, 6 * B - 1):
        mo = rig.check(oracle, [(r, 0, cut), (r, cut, ALL)], pats)
        assert [(x, p) for q, x, p in triples(mo)] == [(x, p) for q, x, p in everything], cut
    # requests that share blocks, a request repeated, a resource of the other parity between them
    reqs = [(r, 100, 300), (r, 200, 2 * B), (S.RANDOM_FIRST, B - 9, 20), (r, 100, 300), (r, 200, 2 * B), (S.RUN, 5, 50)]
    mo = rig.check(oracle, reqs, pats + [b"aaaaa"], crc=True)
    assert mo["req_hits"][0] == mo["req_hits"][3] and mo["req_hits"][1] == mo["req_hits"][4] and mo["req_hits"][5] == 50 and "shared_block" in mo["edges"]
    assert mo["counts"] == (1 + 3 + 2 + 1 + 3 + 1, 3 + 2 + 1, mo["counts"][2])


@pytest.mark.parametrize("fmt", list(FMTS))
def test_statuses_leave_the_other_requests_alone(rigs, oracle, fmt):
    rig = rigs(fmt)
    pats = [S.NEEDLE, b"\x05\x06"]
    reqs = [(S.SOFT_FIRST, 0, 2 * B), (S.RANDOM_FIRST, B, 2 * B), (S.B_MORE, 0, ALL), (S.MIX, 0, ALL), (S.B_LESS, 0, ALL)]
    base = rig.check(oracle, reqs, pats, crc=True)
    assert base["status"] == [0] * 5 and all(base["req_hits"])

    def others(mo, bad):
        assert [s != 0 for s in mo["status"][: len(reqs)]] == [q in bad for q in range(len(reqs))], mo["status"]
        assert mo["req_hits"][: len(reqs)] == [0 if q in bad else h for q, h in enumerate(base["req_hits"])]
    # no such resource
    mo = rig.check(oracle, reqs + [(rig.n, 0, 5), (ALL, 0, ALL)], pats, crc=True)
    assert mo["status"][5:] == [M.ARG, M.ARG]
    others(mo, set())
    # a wrong block count
    bad = rig.first.copy(); bad[S.MIX + 1] += np.uint64(1)
    mo = rig.check(oracle, reqs, pats, first=bad)
    assert mo["status"][3] == M.DATA
    others(mo, {3, 0, 1} & {q for q, s in enumerate(mo["status"]) if s})
    # the budget: requests 0 and 1 cover 2 blocks each as a reader counts them and 3 with the look-ahead
    assert rig.budget(reqs[:2]) == 4 and rig.searched(reqs[:2], 5) == 6
    mo = rig.check(oracle, reqs[:2], pats, blocks_max=5)
    assert mo["status"] == [0, M.ARG] and mo["req_hits"] == [base["req_hits"][0], 0] and "budget_by_lookahead" in mo["edges"]
    assert rig.check(oracle, reqs[:2], pats, blocks_max=6)["status"] == [0, 0]
    # a flipped byte of a raw block: only the checksums see it; and of the look-ahead block alone
    j = int(rig.first[S.SOFT_FIRST])
    assert int(rig.off[j + 2] - rig.off[j + 1]) == B
    hurt = flipped(rig.packed, int(rig.off[j + 1]) + 1000)
    d_hurt = rig.edited(packed=hurt).d_packed
    mo = rig.check(oracle, reqs, pats, crc=True, packed=d_hurt, model_packed=hurt)
    others(mo, {0})
    assert rig.check(oracle, reqs, pats, packed=d_hurt, model_packed=hurt)["status"] == [0] * 5
    hurt = flipped(rig.packed, int(rig.off[j + 2]) + 3)            # block 2 of request 0's resource: its look-ahead
    mo = rig.check(oracle, reqs, pats, crc=True, packed=rig.edited(packed=hurt).d_packed, model_packed=hurt)
    others(mo, {0})
    # a block that does not decode
    at = flip(oracle, rig, j, B, decodes=False)
    hurt = flipped(rig.packed, at)
    if hurt[at] != rig.packed[at] ^ 0x01:                          # (flip() names a byte whose lowest bit it turned)
        hurt = bytes(rig.packed[:at]) + bytes([rig.packed[at] ^ 0x01]) + bytes(rig.packed[at + 1:])
    mo = rig.check(oracle, reqs, pats, packed=rig.edited(packed=hurt).d_packed, model_packed=hurt)
    others(mo, {0})


@pytest.mark.parametrize("fmt", list(FMTS))
def test_a_second_call_and_a_captured_one(oracle, fmt):
    """one searcher: a call, then another with other data and patterns -- nothing of the first in its answer --, then compress and search
    captured in one graph on a stream of its own and replayed after the container's bytes changed"""
    import torch
    import ms_compress_amd as m
    f = FMTS[fmt]
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    bufs = S.buffers(B)
    with torch.cuda.stream(s):
        rig = SearchRig.make(ctx, f, B, bufs)
        reqs = [(S.SOFT_FIRST, 0, ALL), (S.RUN, B - 2, 40), (S.MIX, 5, ALL), (S.B_MORE, 0, ALL)]
        first_pats, second_pats = [b"aa", S.NEEDLE, b"\x01"], [S.NEEDLE[1:], b"\x02\x03", b"aaaa"]
        budget, room = rig.searched(reqs, 5), 2000
        sr = m.BlockSearcher(ctx, f, B, rig.n, rig.nbt, len(reqs), budget, 3, 5, room)
        one = rig.check(oracle, reqs, first_pats, len_max=5, blocks_max=budget, hits_max=room, searcher=sr)
        assert one["count"][0] > room                              # every word of d_hits was written
        other = [b[::-1] for b in bufs]
        rig.load(other); rig.compress(); ctx.stream.synchronize(); rig.pull()
        two = rig.check(oracle, [(S.RANDOM_FIRST, 3, B), (S.RUN, 0, 7), (0, 0, ALL), (S.THREE, 0, ALL)], second_pats, len_max=5, blocks_max=budget, hits_max=room, searcher=sr)
        assert 0 < two["count"][0] < room and two["req_hits"][1] == 7
        # captured: the tensors of a replay stay where they are
        blob, poff = S.pack_patterns(first_pats)
        d_req, d_pat, d_poff = d64(np.array(reqs, dtype=np.uint64), rig.dev), torch.from_numpy(np.frombuffer(blob + bytes(16), dtype=np.uint8).copy()).to(rig.dev), d64(poff, rig.dev)
        d_hits, d_rh, d_cnt = (torch.full((k,), SENT, dtype=torch.int64, device=rig.dev) for k in (2 * room + GUARD, len(reqs) + GUARD, 2 + GUARD))
        d_pst, d_st = (torch.full((k,), SENT32, dtype=torch.int32, device=rig.dev) for k in (3 + GUARD, len(reqs) + GUARD))
        fresh = m.BlockSearcher(ctx, f, B, rig.n, rig.nbt, len(reqs), budget, 3, 5, room)     # its first execution is inside the capture
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rig.compress()
        fresh.search(rig.d_packed, rig.total, rig.d_first, rig.d_boff, rig.d_len, rig.d_crc, d_req, d_pat, d_poff, d_hits, d_rh, d_cnt, d_pst, d_st)
    for k in range(2):
        now = bufs if k == 0 else [bufs[0]] + [b[1:] + b[:1] for b in bufs[1:]]       # other bytes of the same lengths: every hit moves
        with torch.cuda.stream(s):
            rig.load(now)
            for t in (d_hits, d_rh, d_cnt):
                t.fill_(SENT)
            g.replay()
        s.synchronize()
        rig.pull()
        mo = S.model_search(oracle, f, rig.packed, rig.total, rig.first, rig.off, rig.lens, B, rig.nbt, reqs, blob, poff, 5, budget, room, rig.crc)
        u64 = lambda t: t.cpu().numpy().view(np.uint64)
        same_words(u64(d_hits), [w for rec in mo["records"] for w in rec], SENT, ("d_hits of replay", k))
        same_words(u64(d_rh), mo["req_hits"], SENT, "d_req_hits"); same_words(u64(d_cnt), mo["count"], SENT, "d_count")
        same_words(d_st.cpu().numpy(), mo["status"], SENT32, "d_status"); same_words(d_pst.cpu().numpy(), mo["pat_status"], SENT32, "d_pat_status")
        assert mo["status"] == [0] * len(reqs) and mo["count"][0] > 0
    del g
    fresh.close(); sr.close(); rig.close(); ctx.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_tile_boundaries_of_a_large_block(gpu_ctx, oracle, fmt):
    """B = 65536: the needle across every interior tile boundary of the scan (4096 positions), at every split, in a decoded and in a raw
    block, and across the boundary between the two"""
    big = 65536
    rs = np.random.RandomState(99)
    buf = S.soft(rs, big) + rs.bytes(big) + S.soft(rs, 777)
    want = []
    for t in range(1, 33):
        want.append(t * 4096 - 1 - (t % 4))                        # splits 1|4 .. 4|1 by turns
        buf = S.planted(buf, want[-1])
    rig = SearchRig.make(gpu_ctx, FMTS[fmt], big, [buf, b"", S.soft(rs, 4096 + 9)])
    assert [int(x) == big for x in np.diff(rig.off[:3].astype(np.int64))] == [False, True]
    mo = rig.check(oracle, [(0, 0, ALL), (0, 4093, big), (2, 0, ALL), (0, 2 * big - 1, 1)], [S.NEEDLE, buf[3 * 4096 - 100: 3 * 4096 + 100]], crc=True)
    assert [x for q, x, p in triples(mo) if q == 0 and p == 0] == want and mo["req_hits"] == [33, 17, 0, 1] and mo["counts"][1:] == (4, 3)
    rig.close()


def test_host_convenience(gpu_ctx, oracle):
    """blocks_search over a container that takes several calls, and one call whose records do not fit the first time"""
    import ms_compress_amd as m
    f = 3
    bufs = S.buffers(B)
    lens = [len(b) for b in bufs]
    packed, first, off, st = m.blocks_compress(f, bufs, B, ctx=gpu_ctx)
    bcrc, _ = m.blocks_crc(f, bufs, B, ctx=gpu_ctx)
    assert not st.any()
    pats = [S.NEEDLE, b"aa", b"", S.END3[1:], bytes(257)]
    made = []
    real = m.search.BlockSearcher
    try:
        m.search.BlockSearcher = lambda *a: made.append(a[-1]) or real(*a)          # (the hits_max of every searcher the call makes)
        hits, status, pst = m.blocks_search(f, packed, first, off, lens, B, pats, block_crc=bcrc, ctx=gpu_ctx, blocks_max=4, hits_max=5000)
    finally:
        m.search.BlockSearcher = real
    want = sorted((r, x, p) for r, b in enumerate(bufs) for p, pat in enumerate(pats) if 1 <= len(pat) <= 256 for x in S.find_all(b, pat, 0, len(b) - len(pat) + 1))
    assert hits == want and status == [0] * len(bufs) and pst == [0, 0, M.ARG, 0, M.ARG]
    assert sum(len(b) for b in bufs) // B > 3 * 4 and len(made) == 2 and made[0] == 5000 < made[1]      # several calls; one of them overflowed once
    # ranges, one of a resource that does not exist
    hits, status, pst = m.blocks_search(f, packed, first, off, lens, B, [S.NEEDLE], ranges=[(S.SOFT_FIRST, B - 1, 1), (len(bufs), 0, 5), (S.MIX, 0, 3 * B)], ctx=gpu_ctx)
    assert hits == [(S.SOFT_FIRST, B - 1, 0)] and status == [0, M.ARG, 0] and pst == [0]
