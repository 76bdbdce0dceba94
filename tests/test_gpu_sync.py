"""GPU: mscomp_amd_syncer_sync against the model of tests/sync_model.py -- every entry of the outputs compared in sentinel-filled arrays
that are longer than the call may write --, then the header's consequence on the device: the literal runs copied, BlockReader.read with
the call's own d_req / d_req_off, and the batch compared byte for byte. The stores are made by the GPU's blocks_compress / blocks_crc;
the helpers are those of tests/blocks_rig.py, the cases those of sync_model.cases (which tests/test_sync_model.py holds to the
consequence without a device)."""
import zlib

import numpy as np
import pytest

import blocks_model as M
import sync_model as Y
from blocks_rig import Container, ListOuts, d64, flipped, memo, odd_offsets, same_image, FMTS, FILL, SENT32, ENTRY_GUARD

pytestmark = pytest.mark.gpu
SHAPES = (("lznt1", 4096), ("xpress", 4096), ("xpress_huff", 4096), ("xpress", 65536))
EXACT, PREFIXES = ("hit_first", "lit_first", "count"), ("req", "req_off", "lit")


class Rig:
    """a syncer for ``nu`` units of ``room`` bytes and ``nc`` kept candidates against stores of the bounds of ``store``, with its guarded
    outputs and an input buffer the units are loaded into at odd offsets"""

    def __init__(self, store, nu, room, nc, in_total_max=None):
        import torch
        self.m, self.ctx, self.dev, self.fmt, self.B = store.m, store.ctx, store.dev, store.fmt, store.B
        self.nu, self.nc, self.n_res = nu, nc, store.n
        self.in_total_max = room if in_total_max is None else in_total_max
        self.sy = self.m.BlockSyncer(self.ctx, self.fmt, self.B, store.n, store.nbt, nu, self.in_total_max, nc)
        self.outs = ListOuts(self.dev, {"hit_first": nu + 1, "req": 3 * nc, "req_off": nc, "lit_first": nu + 1, "lit": 2 * (nc + nu), "count": 8}, nu)
        self.res_status = torch.full((store.n + ENTRY_GUARD,), SENT32, dtype=torch.int32, device=self.dev)
        self.d_in = torch.zeros(room + 3 * nu + 64, dtype=torch.uint8, device=self.dev)
        self.d_off, self.d_len = d64([], self.dev, nu), d64([], self.dev, nu)

    def load(self, units):
        import torch
        assert len(units) == self.nu
        self.units = [bytes(u) for u in units]
        self.offs, blob = odd_offsets(self.units, self.d_in.numel())
        self.d_in.copy_(torch.from_numpy(blob))
        self.d_off.copy_(d64(self.offs, self.dev, self.nu)); self.d_len.copy_(d64([len(u) for u in units], self.dev, self.nu))
        self.outs.reset(); self.res_status.fill_(SENT32)

    def launch(self, store):
        o = self.outs
        self.sy.sync(store.view(), self.d_in, self.d_off, self.d_len, o["hit_first"], o["req"], o["req_off"], o["lit_first"], o["lit"], o["count"],
                     self.res_status, o.status)

    def compare(self, oracle, store):
        """the outputs against the model, entry for entry; returns the model"""
        mo = Y.model_sync(oracle, self.fmt, store.model(), self.units, self.offs, self.B, self.in_total_max, self.nc)
        want = dict(mo, req_off=[(x,) for x in mo["req_off"]])
        got = self.outs.pull()
        ListOuts.compare(got, want, exact=EXACT, prefixes=PREFIXES)
        assert [int(x) for x in self.res_status.cpu().numpy()] == mo["res_status"] + [SENT32] * ENTRY_GUARD
        assert self.sy.counts() == (mo["count"][2], mo["count"][7], mo["count"][4])
        return mo

    def check(self, oracle, store, units):
        self.load(units)
        self.launch(store)
        self.ctx.stream.synchronize()
        return self.compare(oracle, store)

    def rebuild(self, store, mo):
        """the consequence on the device, from the arrays the call left: literals copied, the hits read by a BlockReader"""
        import torch
        out = torch.full_like(self.d_in, FILL)
        lit = self.outs["lit"].cpu().numpy().view(np.uint64)
        for i in range(mo["count"][5]):
            o, ln = int(lit[2 * i]), int(lit[2 * i + 1])
            out[o: o + ln] = self.d_in[o: o + ln]
        rd = self.m.BlockReader(self.ctx, self.fmt, self.B, store.n, store.nbt, self.nc, self.nc)
        d_cap = d64([self.B] * self.nc, self.dev)
        d_len, d_st = torch.zeros(self.nc, dtype=torch.int64, device=self.dev), torch.zeros(self.nc, dtype=torch.int32, device=self.dev)
        rd.read(store.d_packed, store.d_first, store.d_boff, store.d_len, self.outs["req"], out, self.outs["req_off"], d_cap, d_len, d_st,
                d_block_crc=store.d_crc, packed_len=store.plen)
        self.ctx.stream.synchronize()
        rd.close()
        hits = mo["count"][4]
        assert [int(x) for x in d_st.cpu().numpy()] == [0] * hits + [M.ARG] * (self.nc - hits)       # a slot behind the hits names no resource
        same_image(out.cpu().numpy(), [(self.offs[u], self.units[u]) for u in range(self.nu) if mo["status"][u] == 0], FILL, "the rebuilt batch")

    def close(self):
        self.sy.close()


@pytest.fixture(scope="module")
def made(gpu_ctx):
    """stores and rigs by name, made once"""
    yield from memo()


def the_store(gpu_ctx, made, fmt, B):
    return made((fmt, B, "store"), lambda: Container.make(gpu_ctx, FMTS[fmt], B, Y.store_buffers(B)))


def run_case(oracle, made, store, name, units, nc=None, rebuild=True):
    room = sum(len(u) for u in units)
    nc = 2 * (room // store.B) + 8 if nc is None else nc
    rig = made((store.fmt, store.B, name, nc), lambda: Rig(store, len(units), room, nc))
    mo = rig.check(oracle, store, units)
    if rebuild:
        rig.rebuild(store, mo)
    return mo, rig


@pytest.mark.parametrize("fmt,B", SHAPES)
def test_edits_and_the_cap(gpu_ctx, oracle, made, fmt, B):
    """one byte inserted at the front, five deleted mid-resource, 4 KiB overwritten; then one candidate fewer than the thinned count"""
    store = the_store(gpu_ctx, made, fmt, B)
    units = Y.cases(B)["edits"]
    mo, _ = run_case(oracle, made, store, "edits", units)
    assert mo["status"] == [0, 0, 0] and mo["count"][4] >= 6 and mo["count"][1] == mo["count"][2] == mo["count"][3]
    assert mo["hits"][0][0] == (1, 0, 0) and mo["hits"][2] == [(0, 2, 0)]
    capped, _ = run_case(oracle, made, store, "edits", units, nc=mo["count"][1] - 1)
    assert capped["kept"] == mo["kept"][:-1] and capped["count"][:3] == mo["count"][:2] + [mo["count"][1] - 1]


@pytest.mark.parametrize("fmt,B", SHAPES)
def test_window_seams(gpu_ctx, oracle, made, fmt, B):
    """units of B - 1, B and B + 1 bytes and an empty one, every unit at an odd offset, hits that start at T - 1, T and T + 1 of the scan's
    tile and one behind two tiles less seven: every window straddles tiles"""
    store = the_store(gpu_ctx, made, fmt, B)
    T = store.m.MSCOMP_AMD_SYNC_TILE
    mo, rig = run_case(oracle, made, store, "seams", Y.cases(B)["seams"])
    assert all(o % 2 == 1 for o in rig.offs[:2])
    assert mo["hits"] == [[], [(0, 2, 0)], [(0, 2, 0)], [], [(T - 1, 2, 0)], [(T, 0, 0)], [(T + 1, 2, 0)], [(2 * T - 7, 0, 2)]]
    assert mo["literals"][0] == [(0, B - 1)] and mo["literals"][2] == [(B, 1)] and mo["literals"][3] == [] and mo["literals"][7][-1] == (2 * T - 7 + B, 17)


@pytest.mark.parametrize("fmt,B", SHAPES)
def test_zeros_are_thinned(gpu_ctx, oracle, made, fmt, B):
    """5 B zeros against the store's zero blocks: every position a raw candidate, five survive; the smallest of the five equal rows is
    taken; the same stretch across a tile seam"""
    store = the_store(gpu_ctx, made, fmt, B)
    units = Y.cases(B)["zeros"]
    mo, _ = run_case(oracle, made, store, "zeros0", units[:1])
    assert mo["count"][:5] == [4 * B + 1, 5, 5, 5, 5] and mo["count"][7] == 1
    assert mo["hits"][0] == [(i * B, 1, 0) for i in range(5)] and mo["literals"] == [[]]
    mo, _ = run_case(oracle, made, store, "zeros", units)
    assert [p for p, _, _ in mo["hits"][1]] == [Y.TILE - 100 + i * B for i in range(5)]


@pytest.mark.parametrize("fmt,B", SHAPES[1::2])
def test_forged_collision_and_short_last_block(gpu_ctx, oracle, made, fmt, B):
    """a block with the CRC-32 of a store block and other bytes is kept and refuted; the store's short last block matches nothing"""
    store = the_store(gpu_ctx, made, fmt, B)
    mo, _ = run_case(oracle, made, store, "forged", Y.cases(B)["forged"])
    assert mo["count"][2] == 2 and mo["count"][3] == 1 and mo["hits"] == [[(33 + B + 5, 2, 0)]]
    mo, _ = run_case(oracle, made, store, "short", Y.cases(B)["short"])
    assert mo["hits"] == [[(0, 0, 2)], []]


@pytest.mark.parametrize("fmt", ["lznt1", "xpress_huff"])
def test_damage(gpu_ctx, oracle, made, fmt):
    """a stored byte flipped: the row is refuted and its bytes come out as literals; a resource refused by its block count brings no
    rows; a view without checksums is refused"""
    B = 4096
    store = the_store(gpu_ctx, made, fmt, B)
    A, Z, X = Y.store_buffers(B)
    units = [A, X + Z[:B]]
    hurt = store.edited(packed=flipped(store.packed, int(store.off[1]) + 9))      # row 1: the text block of the mixed resource
    mo, rig = run_case(oracle, made, hurt, "damage", units)
    assert mo["hits"] == [[(0, 0, 0), (2 * B, 0, 2)], [(0, 2, 0), (B, 1, 0)]] and mo["literals"][0] == [(B, B), (3 * B, 17)]
    assert mo["count"][2] == 4 + 1 and mo["count"][3] == 4
    lens = list(store.lens)
    lens[1] += B                                                                  # five blocks for six blocks' worth of bytes
    mo = rig.check(oracle, store.edited(lens=lens), units)
    assert mo["res_status"] == [0, M.DATA, 0] and mo["hits"][1] == [(0, 2, 0)]
    rig.load(units)
    with pytest.raises(store.m.MSCompError) as e:
        rig.launch(store.edited(with_crc=False))
    assert e.value.status == store.m.MSCOMP_ARG_ERROR and rig.outs.untouched()


def test_bounds_and_duplicates(gpu_ctx, oracle, made):
    """a unit over in_total_max is refused and the units in front of it are answered; of two equal store blocks the smaller row is taken"""
    B = 4096
    X = Y.rnd(41, B)
    store = made(("dup",), lambda: Container.make(gpu_ctx, FMTS["xpress"], B, [Y.rnd(42, B) + X, X + X]))
    units = [b"q" + X, X + b"r", X + X]
    rig = Rig(store, 3, sum(len(u) for u in units), 16, in_total_max=2 * B + 2)
    mo = rig.check(oracle, store, units)
    assert mo["status"] == [0, 0, M.ARG] and mo["hits"] == [[(1, 0, 1)], [(0, 0, 1)], []] and mo["literals"][2] == []
    rig.rebuild(store, mo)
    rig.close()


def test_probe_chain_crosses_the_table_end(gpu_ctx, oracle, made):
    """three store blocks whose words all start their walk at the last slot of a 128-slot key table: the claims end in slots 127, 0 and 1,
    and the scan's read-only walk has to follow them around the end, whatever order the claims came in"""
    B, SLOTS, SHIFT = 4096, 128, 25                                             # (n_blocks_table <= 32: 2 * 32 + 64 slots)
    word = lambda b: zlib.crc32(b) ^ zlib.crc32(bytes(B))
    start = lambda b: ((word(b) * 0x9E3779B1) & 0xFFFFFFFF) >> SHIFT
    rs, blocks = np.random.RandomState(20261020), []
    while len(blocks) < 3:
        b = rs.bytes(B)
        if start(b) == SLOTS - 1 and word(b) not in [word(x) for x in blocks]:
            blocks.append(b)
    store = made(("wrap",), lambda: Container.make(gpu_ctx, FMTS["xpress"], B, [b"".join(blocks)]))
    assert store.n == 1 and 3 <= store.nbt <= 32 and [start(b) for b in blocks] == [SLOTS - 1] * 3 and len({word(b) for b in blocks}) == 3
    assert [int(c) for c in store.crc[:3]] == [zlib.crc32(b) for b in blocks]
    unit = b"\x07" + blocks[2] + b"fill2" + blocks[1] + b"fill1" + blocks[0]
    mo, _ = run_case(oracle, made, store, "wrap", [unit])
    assert mo["hits"] == [[(1, 0, 2), (1 + B + 5, 0, 1), (1 + 2 * (B + 5), 0, 0)]] and mo["count"][4] == 3


def test_state_and_graphs(gpu_ctx, oracle, made):
    """a second call on the same object with other data gives the model's answer; the later executions replay the object's graph"""
    B = 4096
    store = the_store(gpu_ctx, made, "xpress", B)
    A, Z, X = Y.store_buffers(B)
    first = Y.cases(B)["edits"]
    other = [X + b"!", Y.rnd(43, len(first[1])), A[B:]]
    rig = Rig(store, 3, sum(len(u) for u in first), 64)
    a = rig.check(oracle, store, first)
    b = rig.check(oracle, store, other)                                         # nothing of the first call in the key table, the flags or the lists
    assert b["hits"] == [[(0, 2, 0)], [], [(0, 0, 1), (B, 0, 2)]] and a["count"] != b["count"]
    for _ in range(3):                                                          # from the second execution on: the graph
        assert rig.check(oracle, store, first)["count"] == a["count"]
    rig.rebuild(store, a)
    rig.close()


def test_first_execution_inside_a_capture():
    """the first execution of a syncer inside a capture of the ctx stream; the graph is replayed on other units in the same arrays"""
    import torch
    import ms_compress_amd as m
    from oracle import loader
    loader.build(); loader.load_oracle()
    B = 4096
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        store = Container.make(ctx, FMTS["lznt1"], B, Y.store_buffers(B))
        first = Y.cases(B)["edits"]
        rig = Rig(store, 3, sum(len(u) for u in first), 64)
        rig.load(first)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rig.launch(store)
    for units in (first, [first[2], first[0][:-1], first[1][: 3 * B]], first):
        with torch.cuda.stream(s):
            rig.load(units)
            g.replay()
        s.synchronize()
        mo = rig.compare(loader, store)
        assert mo["count"][4] >= 4
    with torch.cuda.stream(s):
        rig.rebuild(store, mo)
    del g
    rig.close(); store.close(); ctx.close()


@pytest.mark.parametrize("fmt,B", SHAPES[::3])
def test_host_conveniences(gpu_ctx, oracle, made, fmt, B):
    """blocks_sync answers as the model does; blocks_sync_delta and blocks_sync_patch carry the buffers over"""
    import ms_compress_amd as m
    store = the_store(gpu_ctx, made, fmt, B)
    units = Y.cases(B)["edits"]
    hits, lits, counts, rst, st = m.blocks_sync(store.host(), units, B, ctx=gpu_ctx, fmt=FMTS[fmt])
    mo = Y.model_sync(oracle, FMTS[fmt], store.model(nbt=int(store.first[-1]), plen=store.plen), units, [0] * len(units), B, sum(len(u) for u in units), 1 << 20)
    assert (hits, lits, counts, rst, st) == (mo["hits"], mo["literals"], mo["count"], mo["res_status"], mo["status"])
    recipe, data = m.blocks_sync_delta(store.host(), units, B, ctx=gpu_ctx, fmt=FMTS[fmt])
    assert len(data) == counts[6] and recipe[1] == hits
    assert m.blocks_sync_patch(store.host(), recipe, data, B, ctx=gpu_ctx, fmt=FMTS[fmt]) == [bytes(u) for u in units]
    with pytest.raises(ValueError):
        m.blocks_sync(store.host(), units, B, ctx=gpu_ctx)
