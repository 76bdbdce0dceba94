"""GPU: mscomp_amd_splicer_splice against the model of tests/splice_model.py -- the whole new packed buffer and every entry of the three new
tables, the checksums, the lengths and the statuses compared with sentinel images (so a byte at or behind new_cap, or behind the
container's end, fails) -- on two containers of tests/blocks_rig.Container that hold the same buffers in two orders; where the sources are
healthy also byte for byte against BlockContainer.compress + .crc of the picked data."""
import zlib

import numpy as np
import pytest

import blocks_model as M
import read_model as R
import splice_model as S
from blocks_rig import Container, Splices, d64, memo, FMTS, BLOCKS, FILL, ST_FILL, ALL, MIXED, TEXT, ZEROS5
from splice_model import ORDER2, pick_lists

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rigs(gpu_ctx):
    yield from memo(lambda fmt, B: Splices(gpu_ctx, FMTS[fmt], B))


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_identity(rigs, fmt, B):
    zs = rigs(fmt, B)
    rig = zs.rig[0]
    picks = pick_lists(rig.n)[0]
    for crc in (True, False):
        mo, got = zs.check(picks, rig.nbt, srcs=zs.src[:1], crc=crc)
        assert mo["status"] == [0] * rig.n and mo["new_len"] == rig.lens
        assert (got["first"] == rig.first).all() and (got["off"] == rig.off).all() and bytes(got["image"][: rig.plen]) == rig.packed
        assert crc is False or (got["crc"] == rig.crc).all()


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_delete_reorder_duplicate(rigs, fmt, B):
    zs = rigs(fmt, B)
    picks = pick_lists(zs.rig[0].n)[1]
    nbt = zs.table_for(picks)
    mo, got = zs.check(picks, nbt, srcs=zs.src[:1])
    assert mo["status"] == [0] * len(picks)
    zs.check_consequence(got, zs.data(picks), nbt)


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_merge_two_sources(rigs, fmt, B):
    zs = rigs(fmt, B)
    picks = pick_lists(zs.rig[0].n)[2]                             # by turns from the second container and the first
    assert {s for s, _ in picks} == {0, 1}
    nbt = zs.table_for(picks)
    mo, got = zs.check(picks, nbt)
    assert mo["status"] == [0] * len(picks) and mo["new_len"] == zs.rig[0].lens + [len(zs.rig[1].bufs[0]), zs.rig[0].lens[MIXED]]
    zs.check_consequence(got, zs.data(picks), nbt)


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_rejects(rigs, fmt, B):
    import torch
    zs = rigs(fmt, B)
    rig = zs.rig[0]
    n, lens, nb = rig.n, rig.lens, int(rig.first[-1])
    # rule 1, each cause: the pick is an empty resource, the picks around it are carried
    falling = rig.first.copy(); falling[3] = falling[4] + np.uint64(1)
    beyond = rig.first.copy(); beyond[n] = np.uint64(rig.nbt + 1)
    for picks, src0 in (([(0, 1), (2, 0), (0, 4)], None), ([(0, 1), (0, n), (1, 4)], None), ([(0, 1), (0, 1 << 63), (0, 4)], None), ([(0, 1), (1 << 40, 1), (0, 4)], None),
                        ([(0, 1), (0, 3), (0, 4)], rig.edited(first=falling)), ([(0, 1), (0, n - 1), (0, 4)], rig.edited(first=beyond))):
        mo, got = zs.check(picks, 8, srcs=[src0 or zs.src[0], zs.src[1]])
        assert mo["status"] == [0, M.ARG, 0] and mo["new_len"][1] == 0 and int(got["first"][1]) == int(got["first"][2])
    # rule 2: a length that asks for one block more than the table has
    odd = list(lens); odd[MIXED] += B
    mo, got = zs.check([(0, MIXED), (0, TEXT), (1, 0)], 12, srcs=[rig.edited(lens=odd), zs.src[1]])
    assert mo["status"] == [M.DATA, 0, 0] and mo["new_len"] == [0, lens[TEXT], lens[TEXT]] and list(got["first"]) == [0, 0, 4, 8]
    # rule 3 crossed mid-list: counts 4, 5, 4, 1, 0 against 8 rows; then a table filled to its last row
    mo, got = zs.check([(0, MIXED), (0, ZEROS5), (1, 0), (0, 1), (0, 0)], 8)
    assert mo["status"] == [0, M.ARG, M.ARG, M.ARG, 0] and list(got["first"]) == [0, 4, 4, 4, 4, 4]
    mo, got = zs.check([(0, MIXED), (1, 0)], 8)
    assert mo["status"] == [0, 0] and int(got["first"][-1]) == 8
    mo, got = zs.check([(0, MIXED), (1, 0)], 0)                    # no table at all: d_new_packed is never touched
    assert mo["status"] == [M.ARG, M.ARG] and (got["image"] == FILL).all()
    # rule 7: new_cap inside the second block of the second pick, and at 0
    picks = [(0, TEXT), (1, ORDER2.index(MIXED)), (0, 1), (0, 0)]
    full = zs.check(picks, 12)[0]
    g = int(full["first"][1])
    mo, got = zs.check(picks, 12, cap=int(full["off"][g + 2]) - 1)
    assert mo["status"] == [0, M.BUF, M.BUF, 0] and (got["off"] == full["off"]).all() and (got["image"][int(full["off"][g + 1]):] == FILL).all()
    mo, got = zs.check(picks, 12, cap=0)
    assert mo["status"] == [M.BUF, M.BUF, M.BUF, 0] and (got["image"] == FILL).all()
    # no picks: an empty container, all of the offset and checksum tables written
    mo, got = zs.check([], 5)
    assert list(got["first"]) == [0] and not got["off"].any() and not got["crc"].any()
    zs.check([], 0)
    # a view without checksums beside a non-null d_new_block_crc: refused on the host, nothing written
    outs = zs.outputs(2, 8).tensors()
    sp = zs.m.BlockSplicer(zs.ctx, B, 2, 2, 8)
    with pytest.raises(zs.m.MSCompError) as e:
        sp.splice([zs.src[0].view(), zs.rig[1].view(crc=False)], d64([0, 1, 1, 1], zs.dev), outs[0], outs[1], outs[2], outs[4], outs[5], d_new_block_crc=outs[3])
    assert e.value.status == zs.m.MSCOMP_ARG_ERROR
    sp.close()
    torch.cuda.synchronize()
    assert (outs[0].cpu().numpy() == FILL).all() and (outs[2].cpu().numpy() == -1).all()


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_damage(rigs, fmt, B):
    zs = rigs(fmt, B)
    rig = zs.rig[0]
    j = int(rig.first[MIXED])                                     # block 0 raw, block 1 compressed, block 2 raw, block 3 (17 bytes)
    assert int(rig.off[j + 1] - rig.off[j]) == B
    picks = [(0, TEXT), (0, MIXED), (1, 0), (0, MIXED)]
    # a decreasing source entry, and one beyond packed_len, become empty rows
    falling = rig.off.copy(); falling[j + 2] = falling[j + 1] - np.uint64(1)
    past = rig.off.copy(); past[j + 4:] = np.uint64(rig.plen + 1)
    for bad, row in ((falling, 1), (past, 3)):
        mo, got = zs.check(picks, 16, srcs=[rig.edited(off=bad), zs.src[1]])
        for g in (int(got["first"][1]), int(got["first"][3])):
            assert mo["status"] == [0] * 4 and int(got["off"][g + row + 1]) == int(got["off"][g + row])
    # a flipped stored byte is carried as it is; a reader with checksums answers MSCOMP_DATA_ERROR for exactly the requests that cover it
    hurt = bytearray(rig.packed); hurt[int(rig.off[j]) + 77] ^= 0x01
    mo, got = zs.check(picks, 16, srcs=[rig.edited(packed=bytes(hurt)), zs.src[1]])
    assert mo["status"] == [0] * 4
    nb = int(got["first"][-1])
    reqs = [(0, 0, ALL), (1, 0, 10), (1, B - 1, 1), (1, B, ALL), (2, 0, ALL), (3, B - 5, 10), (3, 2 * B, 40)]
    out, st = zs.m.blocks_read(zs.fmt, got["image"][: int(got["off"][nb])], got["first"], got["off"][: nb + 1], mo["new_len"], B, reqs, ctx=zs.ctx,
                               block_crc=got["crc"][:nb])
    assert st == [0, M.DATA, M.DATA, 0, 0, M.DATA, 0]
    data = zs.data(picks)
    assert [o for o in out if o is not None] == [data[0], data[1][B:], data[2], data[3][2 * B: 2 * B + 40]]


def test_long_runs_and_slice_edges(gpu_ctx):
    """a resource of 310 blocks of 4096 bytes -- random and text by turns, then 150 blocks of zeros (hundreds of rows within one 4096-byte
    slice of the new container), then text -- between two small ones: dropping the first small one shifts every row by a constant that is
    no multiple of 16, dropping the last one leaves one run from offset 0"""
    B = 4096
    long = (M.build({"kind": "mixed", "seed": 21, "mult": 100, "add": 0}, B) + bytes(150 * B) + M.build({"kind": "text", "seed": 22, "mult": 60, "add": 17}, B))
    small = [M.build({"kind": "text", "seed": 23, "mult": 1, "add": 5}, B), M.build({"kind": "random", "seed": 24, "mult": 0, "add": 77}, B)]
    zs = Splices(gpu_ctx, FMTS["xpress"], B, bufs0=[small[0], long, small[1]], bufs1=[small[1]])
    rig = zs.rig[0]
    stored = np.diff(rig.off[: int(rig.first[-1]) + 1].astype(np.int64))
    assert int(rig.first[2] - rig.first[1]) == 311 and len(set(stored.tolist())) > 20 and (stored[120:240] < 64).all()
    for picks in ([(0, 1), (0, 2)], [(0, 0), (0, 1)], [(0, 1)], [(0, 2), (0, 1), (1, 0), (0, 1), (0, 0)]):
        nbt = zs.table_for(picks)
        mo, got = zs.check(picks, nbt)
        assert mo["status"] == [0] * len(picks)
        zs.check_consequence(got, zs.data(picks), nbt)
    zs.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_repeats_and_ping_pong(rigs, fmt):
    """one splicer: three executions (its graph replayed from the second on), then another pick list in the same tensor -- the same arguments,
    the same graph --, then other output buffers -- the graph is captured again; everything is compared each time"""
    B = 4096
    zs = rigs(fmt, B)
    n = zs.rig[0].n
    picks_a, picks_b = pick_lists(n)[2], [(s ^ 1, (r * 5 + 3) % n) for s, r in pick_lists(n)[2]]
    npk, nbt = len(picks_a), max(zs.table_for(picks_a), zs.table_for(picks_b)) + 2
    sp = zs.m.BlockSplicer(zs.ctx, B, 2, npk, nbt)
    srcs = [s.view() for s in zs.src]
    d_pick = d64(np.array(picks_a, dtype=np.uint64).reshape(-1), zs.dev)
    outs = [zs.outputs(npk, nbt), zs.outputs(npk, nbt)]

    def run(o, picks):
        d_new, d_first, d_off, d_crc, d_len, d_st = o.tensors()
        o.fill()
        sp.splice(srcs, d_pick, d_new, d_first, d_off, d_len, d_st, d_new_block_crc=d_crc, new_cap=zs.room)
        mo = S.model_splice([s.model() for s in zs.src], picks, B, nbt, zs.room)
        assert mo["status"] == [0] * npk
        zs.compare(zs.pull(o), mo, npk, nbt)
    for _ in range(3):
        run(outs[0], picks_a)
    d_pick.copy_(d64(np.array(picks_b, dtype=np.uint64).reshape(-1), zs.dev))
    for _ in range(2):
        run(outs[0], picks_b)
    for o in (outs[1], outs[1], outs[0]):
        run(o, picks_b)
    sp.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_compress_crc_splice_read_in_one_captured_graph(oracle, fmt):
    """the container's compress and crc, a splice out of it and a reader's read of the spliced container with checksums, captured together
    -- the splicer's and the reader's first executions inside the capture -- and replayed twice, with other data"""
    import torch
    import ms_compress_amd as m
    f, B = FMTS[fmt], 4096
    base = R.buffers(B)
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        rig = Container.make(ctx, f, B, base)
        dev, n = rig.dev, rig.n
        picks = [(0, MIXED), (0, 0), (0, TEXT), (0, MIXED), (0, ZEROS5), (0, 1)]
        npk = len(picks)
        lens = [rig.lens[r] for _, r in picks]
        room = sum(lens)
        nbt = npk + room // B
        sp = m.BlockSplicer(ctx, B, 1, npk, nbt)
        d_pick = d64(np.array(picks, dtype=np.uint64).reshape(-1), dev)
        d_new = torch.empty(room + 64, dtype=torch.uint8, device=dev)
        d_nfirst, d_noff = torch.zeros(npk + 1, dtype=torch.int64, device=dev), torch.zeros(nbt + 1, dtype=torch.int64, device=dev)
        d_ncrc, d_nlen = torch.zeros(nbt, dtype=torch.int32, device=dev), torch.zeros(npk, dtype=torch.int64, device=dev)
        d_st = torch.zeros(npk, dtype=torch.int32, device=dev)
        reads = [(0, B - 10, 30), (2, 0, ALL), (3, 3 * B, ALL), (4, 0, ALL), (5, 0, 1)]
        caps = [30, lens[2], 17, lens[4], 1]
        ooff, oroom = rig.layout(caps)
        rd = m.BlockReader(ctx, f, B, npk, nbt, len(reads), 16)
        d_rreq, d_ooff, d_ocap = d64(np.array(reads, dtype=np.uint64).reshape(-1), dev), d64(ooff, dev), d64(caps, dev)
        d_olen, d_ost = torch.zeros(len(reads), dtype=torch.int64, device=dev), torch.zeros(len(reads), dtype=torch.int32, device=dev)
        d_out = torch.empty(oroom, dtype=torch.uint8, device=dev)
        src = (rig.d_packed, rig.d_first, rig.d_boff, rig.d_len, rig.d_crc, rig.total, n, rig.nbt)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rig.compress()
        sp.splice([src], d_pick, d_new, d_nfirst, d_noff, d_nlen, d_st, d_new_block_crc=d_ncrc, new_cap=room)
        rd.read(d_new, d_nfirst, d_noff, d_nlen, d_rreq, d_out, d_ooff, d_ocap, d_olen, d_ost, d_block_crc=d_ncrc, packed_len=room)
    for k in range(2):
        bufs = base if k == 0 else [bytes(reversed(b)) for b in base]
        with torch.cuda.stream(s):
            rig.load(bufs)
            d_new.fill_(FILL); d_out.fill_(FILL)
            g.replay()
        s.synchronize()
        data = [bufs[r] for _, r in picks]
        assert not d_st.cpu().numpy().any() and not d_ost.cpu().numpy().any(), k
        assert [int(x) for x in d_nlen.cpu().numpy()] == lens
        image = np.full(oroom, FILL, dtype=np.uint8)
        for o, (r, at, ln), c in zip(ooff, reads, caps):
            image[o: o + c] = np.frombuffer(data[r][at: at + c], dtype=np.uint8)
        assert (d_out.cpu().numpy() == image).all(), k
        packed, first, off, _ = M.model_compress(oracle, f, data, B, room, room)
        assert (d_nfirst.cpu().numpy().view(np.uint64) == first).all() and (d_noff.cpu().numpy().view(np.uint64) == off).all()
        assert bytes(d_new.cpu().numpy()[: len(packed)]) == packed and (d_new.cpu().numpy()[len(packed):] == FILL).all()
        assert (d_ncrc.cpu().numpy().view(np.uint32) == R.block_crcs(data, B, nbt)).all()
    del g
    rd.close(); sp.close()
    rig.close()
    ctx.close()


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_res_crc_of_a_spliced_container(rigs, fmt, B):
    import torch
    zs = rigs(fmt, B)
    picks = pick_lists(zs.rig[0].n)[2]
    npk, nbt = len(picks), zs.table_for(picks) + 3
    mo, got = zs.check(picks, nbt)
    d_new, d_first, d_off, d_crc, d_len, d_st = got["d"]
    d_rcrc = torch.full((npk,), 0x33333333, dtype=torch.int32, device=zs.dev)
    d_rst = torch.full((npk,), ST_FILL, dtype=torch.int32, device=zs.dev)
    zs.m.res_crc_dev(zs.ctx, B, npk, nbt, d_first, d_len, d_crc, d_rcrc, d_rst)
    zs.ctx.stream.synchronize()
    assert not d_rst.cpu().numpy().any()
    assert [int(x) for x in d_rcrc.cpu().numpy().view(np.uint32)] == [zlib.crc32(b) for b in zs.data(picks)]


def test_host_convenience(gpu_ctx):
    import ms_compress_amd as m
    f, B = 3, 4096
    bufs0 = R.buffers(B)
    bufs1 = [bufs0[i] for i in ORDER2]
    cons = []
    for bufs in (bufs0, bufs1):
        packed, first, off, st = m.blocks_compress(f, bufs, B, ctx=gpu_ctx)
        bcrc, _ = m.blocks_crc(f, bufs, B, ctx=gpu_ctx)
        cons.append((packed, first, off, [len(b) for b in bufs], bcrc))
    picks = pick_lists(len(bufs0))[2]
    data = S.picked([bufs0, bufs1], picks)
    new_packed, nfirst, noff, nlen, ncrc, status = m.blocks_splice(cons, picks, B, ctx=gpu_ctx)
    assert status == [0] * len(picks) and nlen == [len(b) for b in data] and ncrc is not None
    out, st = m.blocks_decompress(f, new_packed, nfirst, noff, nlen, B, ctx=gpu_ctx, block_crc=ncrc)
    assert st == [0] * len(picks) and out == data
    plain = m.blocks_splice([c[:4] + (None,) for c in cons], picks[:3] + [(2, 0)], B, ctx=gpu_ctx)
    assert plain[4] is None and plain[5] == [0, 0, 0, M.ARG] and plain[3] == [len(b) for b in data[:3]] + [0]
