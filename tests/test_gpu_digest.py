"""GPU: the block digests against tests/digest_model.py. The digester's column and check over every finalisation corner of the tree; then
mscomp_amd_syncer_sync_digest -- every entry of the outputs in sentinel-filled arrays against model_sync_digest and, on healthy stores,
against what BlockSyncer.sync writes for the same inputs; the consequence rebuilt on the device with BlockReader.read. The stores are
made by the GPU's blocks_compress / blocks_crc and the digester; the rig is the one of tests/test_gpu_sync.py with a digest syncer beside
its syncer."""
import numpy as np
import pytest

import blocks_model as M
import digest_model as G
import sync_model as Y
from blocks_rig import BlockRig, Container, ListOuts, d64, memo, odd_offsets, FMTS, SENT32, ENTRY_GUARD
from test_gpu_sync import Rig, EXACT, PREFIXES

pytestmark = pytest.mark.gpu
DIG_FILL = 0x5A5A5A5A


def pat(n):
    return bytes((i * 7 + 3) & 255 for i in range(n))


# ---- the digester ---------------------------------------------------------------------------------------------------------------------------
class DigRig:
    """a digester for n resources with its input buffer (the resources at odd offsets) and a guarded digest column and status array"""

    def __init__(self, ctx, B, n, in_total_max, room):
        import torch
        import ms_compress_amd as m
        self.ctx, self.B, self.n, self.itm = ctx, B, n, in_total_max
        self.dev = dev = torch.device("cuda", ctx.device)
        self.dg = m.BlockDigester(ctx, B, n, in_total_max)
        self.nbm = self.dg.n_blocks_max
        assert self.nbm == n + in_total_max // B
        self.d_in = torch.zeros(room + 3 * n + 64, dtype=torch.uint8, device=dev)
        self.d_off, self.d_len = d64([], dev, n), d64([], dev, n)
        self.d_dig = torch.full((4 * (self.nbm + ENTRY_GUARD),), DIG_FILL, dtype=torch.int32, device=dev)
        self.d_st = torch.full((n + ENTRY_GUARD,), SENT32, dtype=torch.int32, device=dev)

    def check(self, bufs):
        import torch
        off, blob = odd_offsets(bufs, self.d_in.numel())
        self.d_in.copy_(torch.from_numpy(blob))
        self.d_off.copy_(d64(off, self.dev, self.n)); self.d_len.copy_(d64([len(b) for b in bufs], self.dev, self.n))
        self.d_dig.fill_(DIG_FILL); self.d_st.fill_(SENT32)
        self.dg.blocks(self.d_in, self.d_off, self.d_len, self.d_dig, self.d_st)
        self.ctx.stream.synchronize()
        want, st = G.model_digests(bufs, self.B, self.itm)
        got = self.d_dig.cpu().numpy().view(np.uint32)
        bad = np.nonzero((got[: 4 * self.nbm].reshape(-1, 4) != want).any(axis=1))[0]
        assert bad.size == 0, ("digest of block", int(bad[0]))
        assert (got[4 * self.nbm:] == DIG_FILL).all(), "written behind the column"
        assert [int(x) for x in self.d_st.cpu().numpy()] == [int(x) for x in st] + [SENT32] * ENTRY_GUARD
        return want, st

    def close(self):
        self.dg.close()


def test_known_answers_on_the_device(gpu_ctx):
    """the header's known answers through the host convenience: one resource each, at the block size that holds it"""
    import ms_compress_amd as m
    for data, B in ((b"abc", 4096), (bytes(64), 4096), (pat(1024), 4096), (pat(1025), 4096), (pat(4096), 4096), (pat(65536), 65536)):
        got = m.blocks_digest([data], B, ctx=gpu_ctx)
        assert got.shape == (1, 4) and got[0].tobytes() == G.block_digest(data)


def test_block_lengths_4096(gpu_ctx):
    """every finalisation corner: a leaf that ends inside, at the end of and just behind a 64-byte message block; one leaf (the flag on
    leaf and root), a full leaf, a leaf and a byte; short last blocks; an empty resource; zeros behind the count; then other data
    through the same object (the graph), and a resource past in_total_max"""
    B = 4096
    lens = [1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 0, 3 * 4096 + 17]
    bufs = [Y.rnd(100 + i, n) for i, n in enumerate(lens)]
    total = sum(lens)
    rig = DigRig(gpu_ctx, B, len(lens), total + 2 * B, total)
    want, st = rig.check(bufs)
    nb = sum(-(-n // B) for n in lens)
    assert not st.any() and not want[nb:].any() and want[:nb].any(axis=1).all()
    for _ in range(2):                                                           # from the second execution on: the graph
        rig.check([pat(n) for n in lens])
    rig.check(bufs[::-1])
    rig.close()
    rig = DigRig(gpu_ctx, B, len(lens), total - 1, total)                        # the last resource goes over the bound
    want, st = rig.check(bufs)
    assert list(st) == [0] * (len(lens) - 1) + [M.ARG] and not want[nb - 4:].any()
    rig.close()


@pytest.mark.parametrize("B,n", [(65536, 65536 + 1), (524288, 524288)])
def test_block_lengths_large(gpu_ctx, B, n):
    """16 and 128 compressions in the root; a one-byte last block behind a full one"""
    rig = DigRig(gpu_ctx, B, 1, n, n)
    want, _ = rig.check([Y.rnd(7, n)])
    if n == 524288:
        rig.check([pat(n)])
        assert want.shape == (2, 4)
    rig.close()


def test_n_res_zero(gpu_ctx):
    """a digester without resources: both calls return MSCOMP_OK with nothing to report on"""
    import torch
    import ms_compress_amd as m
    dg = m.BlockDigester(gpu_ctx, 4096, 0, 0)
    assert dg.n_blocks_max == 0
    dg.blocks(None, None, None, None, None)
    dg.check(None, None, None, d64([0], torch.device("cuda", gpu_ctx.device)), None, None, None)
    gpu_ctx.stream.synchronize()
    dg.close()


def test_check(gpu_ctx):
    """behind a GPU decompress, with and without a range: healthy data passes and nothing is written; a flipped output byte or a flipped
    digest word fails its resource only; a resource that is not MSCOMP_OK on entry is left alone"""
    import torch
    import ms_compress_amd as m
    B = 4096
    bufs = Y.store_buffers(B)                                                    # 3 B + 17 mixed, 5 B zeros, one raw block
    n, total = len(bufs), sum(len(b) for b in bufs)
    rig = BlockRig(gpu_ctx, FMTS["xpress"], B, n, total)
    rig.load(bufs); rig.compress(); rig.set_out([len(b) + 9 for b in bufs])
    dg = m.BlockDigester(gpu_ctx, B, n, total)
    d_dig = torch.zeros(4 * dg.n_blocks_max, dtype=torch.int32, device=rig.dev)
    d_st = torch.zeros(n, dtype=torch.int32, device=rig.dev)
    dg.blocks(rig.d_in, rig.d_off, rig.d_len, d_dig, d_st)
    gpu_ctx.stream.synchronize()
    dig = d_dig.cpu().numpy().view(np.uint32).reshape(-1, 4).copy()
    assert (dig == G.model_digests(bufs, B, total)[0]).all()
    first, first_t = rig.d_first.cpu().numpy().view(np.uint64), rig.d_first

    def held(ranges, d_dig, st_in, olen_in):
        rig.d_dst[:n] = torch.tensor(st_in, dtype=torch.int32, device=rig.dev); rig.d_olen[:n] = torch.tensor(olen_in, dtype=torch.int64, device=rig.dev)
        before = rig.d_out.clone()
        dg.check(rig.d_out, rig.d_ooff, rig.d_len, first_t, d_dig, rig.d_olen, rig.d_dst, d_range=None if ranges is None else rig.d_range)
        gpu_ctx.stream.synchronize()
        want = G.model_check(before.cpu().numpy(), rig.ooff, rig.lens, first, d_dig.cpu().numpy().view(np.uint32), st_in, olen_in, B, total, ranges)
        got = ([int(x) for x in rig.d_dst.cpu().numpy()[:n]], [int(x) for x in rig.d_olen.cpu().numpy()[:n]])
        assert got == want, (got, want)
        assert torch.equal(before, rig.d_out), "check wrote to the output"
        return got
    for ranges in (None, [(1, 2), (0, 9), (0, 1)]):
        out, olen, st = rig.decompress(ranges)
        st, olen = [int(x) for x in st], [int(x) for x in olen]
        assert st == [0, 0, 0]
        assert held(ranges, d_dig, st, olen) == (st, olen)                       # healthy
        at = rig.ooff[1] + B + 5                                                 # a byte of the second block in range of resource 1
        rig.d_out[at] ^= 0xFF
        assert held(ranges, d_dig, st, olen) == ([0, M.DATA, 0], [olen[0], 0, olen[2]])
        rig.d_out[at] ^= 0xFF
        stale = d_dig.clone()
        stale[4 * (int(first[0]) + 1) + 3] ^= 1 << 30                            # block 1 of resource 0: in range both times
        assert held(ranges, stale, st, olen) == ([M.DATA, 0, 0], [0, olen[1], olen[2]])
        rig.d_out[rig.ooff[2] + 1] ^= 0xFF                                       # not MSCOMP_OK on entry: not read, not written
        assert held(ranges, d_dig, [0, 0, M.BUF], [olen[0], olen[1], 123]) == ([0, 0, M.BUF], [olen[0], olen[1], 123])
    dg.close(); rig.close()


# ---- the digest syncer ----------------------------------------------------------------------------------------------------------------------
def digests_of(store):
    """(device column, host rows) of a Container's data through a BlockDigester of its bounds, held to the model"""
    import torch
    dg = store.m.BlockDigester(store.ctx, store.B, store.n, store.total)
    assert dg.n_blocks_max == store.nbt
    d_dig = torch.zeros(4 * store.nbt + 4, dtype=torch.int32, device=store.dev)
    d_st = torch.zeros(max(1, store.n), dtype=torch.int32, device=store.dev)
    dg.blocks(store.d_in, store.d_off, store.d_len, d_dig, d_st)
    store.ctx.stream.synchronize()
    dg.close()
    dig = d_dig.cpu().numpy().view(np.uint32)[: 4 * store.nbt].reshape(-1, 4).copy()
    assert not d_st.cpu().numpy().any() and (dig == G.store_digests(store.bufs, store.B, store.nbt)).all()
    return d_dig, dig


class DRig(Rig):
    """tests/test_gpu_sync.py's rig with a digest syncer of the same bounds beside its syncer: both write the same guarded outputs"""

    def __init__(self, store, nu, room, nc, in_total_max=None):
        super().__init__(store, nu, room, nc, in_total_max)
        self.dsy = self.m.BlockSyncer.for_digest(self.ctx, self.B, store.n, store.nbt, nu, self.in_total_max, nc)

    def launch_digest(self, store, d_dig, view=None):
        o = self.outs
        self.dsy.sync_digest(store.view() if view is None else view, d_dig, self.d_in, self.d_off, self.d_len, o["hit_first"], o["req"], o["req_off"],
                             o["lit_first"], o["lit"], o["count"], self.res_status, o.status)

    def pull(self):
        self.ctx.stream.synchronize()
        got = self.outs.pull()
        got["res_status"] = [int(x) for x in self.res_status.cpu().numpy()]
        return got

    def compare_digest(self, store, dig):
        """the outputs the digest syncer left against the model, entry for entry; returns (model, outputs)"""
        got = self.pull()
        mo = G.model_sync_digest(store.model(), dig, self.units, self.offs, self.B, self.in_total_max, self.nc)
        ListOuts.compare(got, dict(mo, req_off=[(x,) for x in mo["req_off"]]), exact=EXACT, prefixes=PREFIXES)
        assert got["res_status"] == mo["res_status"] + [SENT32] * ENTRY_GUARD
        assert mo["count"][7] == mo["count"][2] and self.dsy.counts() == (mo["count"][2], mo["count"][2], mo["count"][4])
        return mo, got

    def check(self, store, d_dig, dig, units, healthy=True, view=None):
        """sync_digest against the model and -- on a healthy store -- against sync in the same arrays: every output but count[7]"""
        self.load(units)
        self.launch_digest(store, d_dig, view)
        mo, got = self.compare_digest(store, dig)
        if healthy:
            self.outs.reset(); self.res_status.fill_(SENT32)
            self.launch(store)
            plain = self.pull()
            assert plain["count"][7] <= got["count"][7]                          # distinct rows decoded, against windows hashed
            plain["count"][7] = got["count"][7]
            assert plain == got
        return mo, got

    def close(self):
        super().close()
        self.dsy.close()


@pytest.fixture(scope="module")
def made(gpu_ctx):
    """stores, their digest columns and rigs by name, made once"""
    yield from memo()


def the_store(gpu_ctx, made, fmt, B):
    store = made((fmt, B, "store"), lambda: Container.make(gpu_ctx, FMTS[fmt], B, Y.store_buffers(B)))
    return store, made((fmt, B, "digests"), lambda: digests_of(store))


def run_case(made, store, digs, name, units, nc=None):
    room = sum(len(u) for u in units)
    nc = 2 * (room // store.B) + 8 if nc is None else nc
    rig = made((store.fmt, store.B, name, nc), lambda: DRig(store, len(units), room, nc))
    mo, got = rig.check(store, digs[0], digs[1], units)
    rig.rebuild(store, mo)
    return mo, got, rig


@pytest.mark.parametrize("fmt,B", [("xpress", 4096), ("xpress", 65536)])
def test_sync_cases(gpu_ctx, made, fmt, B):
    """the cases of sync_model.cases against the model, against sync, rebuilt on the device; the capped call too"""
    store, digs = the_store(gpu_ctx, made, fmt, B)
    cases = Y.cases(B)
    T = Y.TILE
    mo, _, _ = run_case(made, store, digs, "edits", cases["edits"])
    assert mo["status"] == [0, 0, 0] and mo["count"][4] >= 6 and mo["count"][1] == mo["count"][2] == mo["count"][3] == mo["count"][7]
    capped, _, _ = run_case(made, store, digs, "edits", cases["edits"], nc=mo["count"][1] - 1)
    assert capped["kept"] == mo["kept"][:-1] and capped["count"][:3] == mo["count"][:2] + [mo["count"][1] - 1]
    mo, _, rig = run_case(made, store, digs, "seams", cases["seams"])
    assert all(o % 2 == 1 for o in rig.offs[:2])
    assert mo["hits"] == [[], [(0, 2, 0)], [(0, 2, 0)], [], [(T - 1, 2, 0)], [(T, 0, 0)], [(T + 1, 2, 0)], [(2 * T - 7, 0, 2)]]
    mo, _, _ = run_case(made, store, digs, "zeros", cases["zeros"])
    assert mo["hits"][0] == [(i * B, 1, 0) for i in range(5)] and [p for p, _, _ in mo["hits"][1]] == [T - 100 + i * B for i in range(5)]
    assert mo["count"][7] == 10                                                  # ten windows hashed where sync decodes one row
    mo, _, _ = run_case(made, store, digs, "forged", cases["forged"])             # same CRC-32, other bytes: kept, and refuted by the digest
    assert mo["count"][2] == 2 and mo["count"][3] == 1 and mo["hits"] == [[(33 + B + 5, 2, 0)]]
    mo, _, _ = run_case(made, store, digs, "short", cases["short"])
    assert mo["hits"] == [[(0, 0, 2)], []]


def test_another_codec_same_digests_same_answer(gpu_ctx, made):
    """the digests are over the data: the store written by another codec has the same column and the call the same answer"""
    B = 4096
    store, digs = the_store(gpu_ctx, made, "xpress", B)
    other, odigs = the_store(gpu_ctx, made, "lznt1", B)
    assert (digs[1] == odigs[1]).all() and other.packed != store.packed
    units = Y.cases(B)["edits"]
    _, a, _ = run_case(made, store, digs, "edits", units)
    _, b, _ = run_case(made, other, odigs, "edits", units)
    assert a == b
    _, c, _ = run_case(made, other, digs, "edits", units)                         # ... and takes the other store's column as its own
    assert c == a


def test_never_reads_the_stores_bytes(gpu_ctx, made):
    """d_packed replaced by a buffer of fill bytes, and by NULL: identical outputs"""
    import torch
    B = 4096
    store, digs = the_store(gpu_ctx, made, "xpress", B)
    units = Y.cases(B)["edits"]
    room = sum(len(u) for u in units)
    rig = made(("blind",), lambda: DRig(store, len(units), room, 64))
    _, want = rig.check(store, digs[0], digs[1], units)
    v = store.view()
    for d_packed in (torch.full_like(store.d_packed, 0xEE), None):
        _, got = rig.check(store, digs[0], digs[1], units, healthy=False, view=(d_packed,) + tuple(v[1:]))
        assert got == want


def test_stale_digest(gpu_ctx, made):
    """one digest word flipped: that row's candidates are refuted and its bytes come out as literals"""
    B = 4096
    store, digs = the_store(gpu_ctx, made, "xpress", B)
    A, Z, X = Y.store_buffers(B)
    units = [A, X + Z[:B]]
    rig = made(("stale",), lambda: DRig(store, 2, sum(len(u) for u in units), 32))
    stale = digs[0].clone()
    stale[4 * 1 + 2] ^= 0x100                                                    # table row 1: block 1 of the mixed resource
    dig = digs[1].copy()
    dig[1, 2] ^= 0x100
    mo, _ = rig.check(store, stale, dig, units, healthy=False)
    assert mo["hits"] == [[(0, 0, 0), (2 * B, 0, 2)], [(0, 2, 0), (B, 1, 0)]] and mo["literals"][0] == [(B, B), (3 * B, 17)]
    assert mo["count"][2] == 4 + 1 and mo["count"][3] == 4
    rig.rebuild(store, mo)                                                       # the recipe is valid, only poorer


def test_kinds_nulls_and_an_empty_store(gpu_ctx, made):
    """the wrong call on each kind is refused with nothing launched; so is a null digest column, a null list and a view without
    checksums; a store without resources answers with literal runs alone"""
    import torch
    import ms_compress_amd as m
    B = 4096
    store, digs = the_store(gpu_ctx, made, "xpress", B)
    units = Y.cases(B)["short"]
    rig = made(("kinds",), lambda: DRig(store, 2, sum(len(u) for u in units), 16))
    rig.load(units)
    o = rig.outs
    tail = (rig.d_in, rig.d_off, rig.d_len, o["hit_first"], o["req"], o["req_off"], o["lit_first"], o["lit"], o["count"], rig.res_status, o.status)
    calls = (lambda: rig.sy.sync_digest(store.view(), digs[0], *tail),           # a syncer made with a format
             lambda: rig.dsy.sync(store.view(), *tail),                          # a digest syncer
             lambda: rig.dsy.sync_digest(store.view(), None, *tail),
             lambda: rig.dsy.sync_digest(store.view(), digs[0], *tail[:3], None, *tail[4:]),
             lambda: rig.dsy.sync_digest(store.view(crc=False), digs[0], *tail))
    for call in calls:
        with pytest.raises(m.MSCompError) as e:
            call()
        assert e.value.status == m.MSCOMP_ARG_ERROR
    gpu_ctx.stream.synchronize()
    assert rig.outs.untouched() and set(int(x) for x in rig.res_status.cpu().numpy()) == {SENT32}
    # n_res = 0
    unit = Y.rnd(5, B + 9)
    sy = m.BlockSyncer.for_digest(gpu_ctx, B, 0, 0, 1, len(unit), 4)
    outs = ListOuts(rig.dev, {"hit_first": 2, "req": 12, "req_off": 4, "lit_first": 2, "lit": 10, "count": 8}, 1)
    d_in = torch.zeros(len(unit) + 64, dtype=torch.uint8, device=rig.dev)
    d_in[3: 3 + len(unit)] = torch.from_numpy(np.frombuffer(unit, dtype=np.uint8).copy()).to(rig.dev)
    empty = (None, d64([0], rig.dev), d64([0], rig.dev), None, torch.zeros(1, dtype=torch.int32, device=rig.dev), 0, 0, 0)
    sy.sync_digest(empty, None, d_in, d64([3], rig.dev), d64([len(unit)], rig.dev), outs["hit_first"], outs["req"], outs["req_off"], outs["lit_first"],
                   outs["lit"], outs["count"], None, outs.status)
    gpu_ctx.stream.synchronize()
    outs.against({"hit_first": [0, 0], "lit_first": [0, 1], "count": [0, 0, 0, 0, 0, 1, len(unit), 0], "status": [0], "req": [], "req_off": [],
                  "lit": [(3, len(unit))]}, exact=EXACT, prefixes=PREFIXES)
    assert sy.counts() == (0, 0, 0)
    sy.close()


def test_state_and_graphs(gpu_ctx, made):
    """a second call on the same object with other data gives the model's answer; the later executions replay the object's graph"""
    B = 4096
    store, digs = the_store(gpu_ctx, made, "xpress", B)
    A, Z, X = Y.store_buffers(B)
    first = Y.cases(B)["edits"]
    other = [X + b"!", Y.rnd(43, len(first[1])), A[B:]]
    rig = DRig(store, 3, sum(len(u) for u in first), 64)
    a, _ = rig.check(store, digs[0], digs[1], first, healthy=False)
    b, _ = rig.check(store, digs[0], digs[1], other, healthy=False)              # nothing of the first call in the key table, the flags or the digests
    assert b["hits"] == [[(0, 2, 0)], [], [(0, 0, 1), (B, 0, 2)]] and a["count"] != b["count"]
    for _ in range(3):                                                           # from the second execution on: the graph
        assert rig.check(store, digs[0], digs[1], first, healthy=False)[0]["count"] == a["count"]
    rig.rebuild(store, a)
    rig.close()


def test_first_execution_inside_a_capture():
    """the first execution of a digest syncer inside a capture of the ctx stream; the graph is replayed on other units in the same arrays"""
    import torch
    import ms_compress_amd as m
    B = 4096
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        store = Container.make(ctx, FMTS["lznt1"], B, Y.store_buffers(B))
        d_dig, dig = digests_of(store)
        first = Y.cases(B)["edits"]
        rig = DRig(store, 3, sum(len(u) for u in first), 64)
        rig.load(first)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rig.launch_digest(store, d_dig)
    for units in (first, [first[2], first[0][:-1], first[1][: 3 * B]], first):
        with torch.cuda.stream(s):
            rig.load(units)
            g.replay()
        s.synchronize()
        mo, _ = rig.compare_digest(store, dig)
        assert mo["count"][4] >= 4
    with torch.cuda.stream(s):
        rig.rebuild(store, mo)
    del g
    rig.close(); store.close(); ctx.close()


def test_host_conveniences(gpu_ctx, made):
    """blocks_sync with a digest column answers as the model does, without a format; delta and patch carry the buffers over"""
    import ms_compress_amd as m
    B = 4096
    store, digs = the_store(gpu_ctx, made, "xpress", B)
    units = Y.cases(B)["edits"]
    host = store.host()
    dig = digs[1][: int(store.first[-1])]
    assert (m.blocks_digest(store.bufs, B, ctx=gpu_ctx) == dig).all()
    hits, lits, counts, rst, st = m.blocks_sync(host, units, B, ctx=gpu_ctx, block_digest=dig)
    mo = G.model_sync_digest(store.model(nbt=int(store.first[-1]), plen=store.plen), dig, units, [0] * len(units), B, sum(len(u) for u in units), 1 << 20)
    assert (hits, lits, counts, rst, st) == (mo["hits"], mo["literals"], mo["count"], mo["res_status"], mo["status"])
    recipe, data = m.blocks_sync_delta(host, units, B, ctx=gpu_ctx, block_digest=dig)
    assert len(data) == counts[6] and recipe[1] == hits
    assert m.blocks_sync_patch(host, recipe, data, B, ctx=gpu_ctx, fmt=FMTS["xpress"], block_digest=dig) == [bytes(u) for u in units]
    with pytest.raises(ValueError):
        m.blocks_sync(host, units, B, ctx=gpu_ctx)
