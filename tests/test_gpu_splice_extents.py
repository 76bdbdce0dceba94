"""GPU: mscomp_amd_splicer_splice_extents against the model of tests/extents_model.py -- the whole new packed buffer and every entry of the
three new tables, the checksums, the lengths and the statuses compared with sentinel images, as tests/test_gpu_splice.py does for picks --
on two containers of tests/blocks_rig.Container: the buffers of tests/extents_model.py (the lengths 0, 1, B - 1, B, B + 1, 3 B, 3 B + 5,
3 B + 17 and 5 B) and the same reversed. Where the sources are healthy also byte for byte against BlockContainer.compress + .crc of the
concatenated extent data."""
import zlib

import numpy as np
import pytest

import blocks_model as M
import extents_model as X
from blocks_rig import Container, Extents, Splices, d64, memo, FMTS, BLOCKS, FILL, ST_FILL, ALL
from extents_model import buffers, healthy_lists, in1, ONE, BP1, MIXED, ZEROS5, TEXT, X3B, X3B5

pytestmark = pytest.mark.gpu
HEALTHY = [(0, TEXT, 1, 2)]                                     # beside every refused resource: two blocks that must come through
HEALTHY_F = [(1, 0, 0, 2)]                                      # the same for the `filler` containers


@pytest.fixture(scope="module")
def rigs(gpu_ctx):
    yield from memo(lambda fmt, B: Extents(gpu_ctx, FMTS[fmt], B))


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_identity_is_the_source_and_what_splice_gives(rigs, fmt, B):
    zs = rigs(fmt, B)
    rig = zs.rig[0]
    resources = healthy_lists(rig.n)["identity"]
    for crc in (True, False):
        mo, got = zs.check(resources, rig.nbt, srcs=zs.src[:1], crc=crc)
        assert mo["status"] == [0] * rig.n and mo["new_len"] == rig.lens
        assert (got["first"] == rig.first).all() and (got["off"] == rig.off).all() and bytes(got["image"][: rig.plen]) == rig.packed
        assert crc is False or (got["crc"] == rig.crc).all()
        _, picked = Splices.check(zs, [(0, r) for r in range(rig.n)], rig.nbt, srcs=zs.src[:1], crc=crc)
        for k in ("image", "first", "off", "crc", "new_len", "status"):
            assert np.array_equal(got[k], picked[k]), k


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_join_split_cut_insert_duplicate_empties(rigs, fmt, B):
    zs = rigs(fmt, B)
    lists = healthy_lists(zs.rig[0].n)
    for name in ("join", "split", "cut_middle", "insert", "duplicate", "empties", "short_last"):
        resources = lists[name]
        nbt = zs.table_for(resources)
        mo, got = zs.check(resources, nbt)
        data = zs.data(resources)
        assert mo["status"] == [0] * len(resources) and mo["new_len"] == [len(b) for b in data], name
        zs.check_consequence(got, data, nbt)
    assert [len(b) for b in zs.data(lists["join"])] == [6 * B + 5] and [len(b) for b in zs.data(lists["split"])] == [2 * B, B + 5]
    assert [len(b) for b in zs.data(lists["empties"])] == [0, 1, 0, 0, 0]


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_rejects(rigs, fmt, B):
    zs = rigs(fmt, B)
    rig = zs.rig[0]
    n = rig.n
    two = 2 * B
    # rules 1 and 3, each cause: the resource is empty, the one beside it is carried
    for bad in ((2, 0, 0, None), (1 << 40, 0, 0, None), (0, n, 0, None), (1, 1 << 63, 0, 1), (0, X3B, 4, None), (0, X3B, 4, 0), (0, X3B, 1, 3), (0, X3B5, 4, 1)):
        for resources in ([[bad], HEALTHY], [HEALTHY, [(0, X3B, 0, 1), bad]]):
            mo, got = zs.check(resources, 8)
            k = resources.index(HEALTHY)
            assert mo["status"][1 - k] == M.ARG and mo["status"][k] == 0 and mo["new_len"][k] == two and mo["new_len"][1 - k] == 0, bad
            assert int(got["first"][2]) == 2
    # rule 1 from a broken source table, rule 2 from a wrong length
    falling = rig.first.copy(); falling[3] = falling[4] + np.uint64(1)
    odd = list(rig.lens); odd[MIXED] += B
    for src0, bad, st in ((rig.edited(first=falling), (0, 3, 0, None), M.ARG), (rig.edited(lens=odd), (0, MIXED, 0, 1), M.DATA)):
        mo, got = zs.check([[(0, X3B, 0, 1), bad], HEALTHY], 8, srcs=[src0, zs.src[1]])
        assert mo["status"] == [st, 0] and mo["new_len"] == [0, two] and list(got["first"]) == [0, 0, 2]
    # rule 4: a B + 1 resource in front of another extent, and as the last one
    mo, got = zs.check([[(0, BP1, 0, None), (0, X3B, 0, 1)], HEALTHY, [(0, X3B, 0, 1), (0, BP1, 0, None), (0, X3B, 3, None)]], 8)
    assert mo["status"] == [M.ARG, 0, 0] and mo["new_len"] == [0, two, two + 1] and list(got["first"]) == [0, 0, 2, 5]
    # rule 0: a falling d_ext_first, and one that ends beyond n_ext -- everything zero, nothing else written
    for kw in ({"ext_first": [0, 2, 1, 3]}, {"n_ext": 2}):
        mo, got = zs.check([[(0, 1, 0, None)], HEALTHY, [(0, 0, 0, None)]], 8, **kw)
        assert mo["status"] == [M.ARG] * 3 and not got["first"].any() and not got["off"].any() and not got["crc"].any() and (got["image"] == FILL).all()
    # rule 6 crossed in the middle: counts 2, 4, 2, 1, 0 against 5 rows; a table filled to its last row; no table at all
    mo, got = zs.check([HEALTHY, [(0, MIXED, 0, None)], HEALTHY, [(0, ONE, 0, None)], [(0, X3B, 0, 0)]], 5)
    assert mo["status"] == [0, M.ARG, M.ARG, M.ARG, 0] and list(got["first"]) == [0, 2, 2, 2, 2, 2]
    mo, got = zs.check([HEALTHY, [(1, in1(X3B), 0, None)]], 5)
    assert mo["status"] == [0, 0] and int(got["first"][-1]) == 5
    mo, got = zs.check([HEALTHY, []], 0)
    assert mo["status"] == [M.ARG, 0] and (got["image"] == FILL).all()
    # capacity: new_cap one byte short of the last block, and 0
    resources = [HEALTHY, [(0, X3B5, 2, None)], [(0, ONE, 0, None)], []]
    full = zs.check(resources, 6)[0]
    mo, got = zs.check(resources, 6, cap=int(full["off"][4]) - 1)
    assert mo["status"] == [0, M.BUF, M.BUF, 0] and (got["off"] == full["off"]).all() and (got["image"][int(full["off"][3]):] == FILL).all()
    mo, got = zs.check(resources, 6, cap=0)
    assert mo["status"] == [M.BUF, M.BUF, M.BUF, 0] and (got["image"] == FILL).all()
    # a damaged off entry is an empty row
    j = int(rig.first[TEXT])
    hurt = rig.off.copy(); hurt[j + 2] = hurt[j + 1] - np.uint64(1)
    mo, got = zs.check([HEALTHY, [(0, TEXT, 0, None)]], 8, srcs=[rig.edited(off=hurt), zs.src[1]])
    assert mo["status"] == [0, 0] and int(got["off"][1]) == int(got["off"][0]) and int(got["off"][4]) == int(got["off"][3])
    # no resources: an empty container, all of the offset and checksum tables written
    mo, got = zs.check([], 5)
    assert list(got["first"]) == [0] and not got["off"].any() and not got["crc"].any()
    zs.check([], 0)


@pytest.fixture(scope="module")
def filler(gpu_ctx):
    """B = 4096: one compressible resource of 2 T + 16 blocks (sixteen text blocks over and over), a B + 1 resource and a small one"""
    B, T = 4096, 1024
    text = M.build({"kind": "text", "seed": 41, "mult": 16, "add": 0}, B)
    big = text * ((2 * T + 16) // 16)
    zs = Extents(gpu_ctx, FMTS["xpress"], B, bufs0=[big, M.build({"kind": "text", "seed": 42, "mult": 1, "add": 1}, B)],
                 bufs1=[M.build({"kind": "mixed", "seed": 43, "mult": 2, "add": 9}, B)])
    yield zs
    zs.close()


def test_row_tile_edges(filler):
    """T - 1, T, T + 1 and 2 T + 1 new rows, in tables that end with the rows and in ones that go on behind them"""
    import ms_compress_amd as m
    zs, T = filler, m.MSCOMP_AMD_SPLICE_ROW_TILE
    assert T == 1024 and len(zs.rig[0].bufs[0]) == (2 * T + 16) * zs.B
    for rows, nbt in ((T - 1, T - 1), (T - 1, T), (T, T), (T, T + 1), (T + 1, T + 1), (T + 1, 2 * T), (2 * T + 1, 2 * T + 1), (2 * T + 1, 2 * T + 5)):
        mo, got = zs.check([[(0, 0, 3, rows - 3)], [(1, 0, 0, None)]], nbt)
        assert mo["status"] == [0, 0] and int(got["first"][-1]) == rows and mo["new_len"] == [(rows - 3) * zs.B, 2 * zs.B + 9]
    # the capacity falls inside the second tile: the rows in front of it are moved, nothing behind
    full = zs.check([[(0, 0, 0, T + 9)], [(1, 0, 0, None)]], T + 12)[0]
    mo, got = zs.check([[(0, 0, 0, T + 9)], [(1, 0, 0, None)]], T + 12, cap=int(full["off"][T + 5]) - 1)
    assert mo["status"] == [M.BUF, M.BUF] and (got["image"][int(full["off"][T + 4]):] == FILL).all()


def test_extent_tile_edges(filler):
    """DV_THREADS + 1 extents in one resource, and DV_THREADS + 1 resources of one extent each: the extent pass works in tiles of 1024"""
    zs, E = filler, 1025
    one = [(0, 0, (7 * i) % 2000, 1) for i in range(E)]
    mo, got = zs.check([HEALTHY_F, one, HEALTHY_F], E + 4)
    assert mo["status"] == [0, 0, 0] and mo["new_len"] == [2 * zs.B, E * zs.B, 2 * zs.B]
    # a short extent in the first tile with a non-empty one behind it in the second; short as the very last one; a bad one in the second tile
    for k, bad, st, ln in ((5, (0, 1, 0, None), M.ARG, 0), (E - 1, (0, 1, 0, None), 0, E * zs.B + 1), (E - 1, (0, 0, 3000, 1), M.ARG, 0), (E - 1, (0, 1, 1, None), 0, (E - 1) * zs.B + 1)):
        exts = list(one); exts[k] = bad
        mo, got = zs.check([HEALTHY_F, exts, HEALTHY_F], E + 5)
        assert mo["status"] == [0, st, 0] and mo["new_len"] == [2 * zs.B, ln, 2 * zs.B], (k, bad)
    many = [[(0, 0, (5 * i) % 2000, 1 + i % 2)] for i in range(E)]
    many[1023] = [(0, 0, 4000, 1)]; many[1024] = [(0, 1, 0, None)]; many[3] = [(2, 0, 0, 1)]; many[500] = []
    mo, got = zs.check(many, 2 * E)
    assert [q for q, s in enumerate(mo["status"]) if s] == [3, 1023] and mo["new_len"][1024] == zs.B + 1 and mo["new_len"][1022] == zs.B
    mo, got = zs.check(many, 700)                                 # the table is crossed in the middle of the first tile of resources
    assert mo["status"][-1] == M.ARG and mo["status"][500] == 0 and int(got["first"][-1]) <= 700



@pytest.mark.parametrize("fmt", list(FMTS))
def test_repeats_and_a_changed_view(rigs, fmt):
    """one splicer: two executions with equal arguments (its graph replayed), another extent list in the same tensors, then a view whose
    table changed -- the graph is captured again; everything is compared each time. The same splicer then serves splice()."""
    B = 4096
    zs = rigs(fmt, B)
    lists = healthy_lists(zs.rig[0].n)
    res_a = lists["join"] + lists["split"] + lists["insert"]
    res_b = lists["duplicate"] + lists["cut_middle"] + [[], [(1, 3, 0, 1)]]
    n_res, n_ext, nbt = 4, 8, max(zs.table_for(res_a), zs.table_for(res_b)) + 2
    sp = zs.m.BlockSplicer.for_extents(zs.ctx, B, 2, n_res, n_ext, nbt)
    outs = zs.outputs(n_res, nbt)
    ef_a, ext_a = X.flat(res_a)
    d_ef, d_ext = d64(ef_a, zs.dev), d64(np.array(ext_a + [(0, 0, 0, 0)] * (n_ext - len(ext_a)), dtype=np.uint64).reshape(-1), zs.dev)
    j = int(zs.rig[0].first[X3B5])
    hurt = zs.rig[0].off.copy(); hurt[j + 1] = hurt[j] - np.uint64(1)

    def run(resources, srcs):
        d_new, d_first, d_off, d_crc, d_len, d_st = outs.tensors()
        outs.fill()
        ef, ext = X.flat(resources)
        d_ef.copy_(d64(ef, zs.dev)); d_ext[: 4 * len(ext)] = d64(np.array(ext, dtype=np.uint64).reshape(-1), zs.dev)
        sp.splice_extents([s.view() for s in srcs], d_ef, d_ext, d_new, d_first, d_off, d_len, d_st, d_new_block_crc=d_crc, new_cap=zs.room)
        mo = X.model_splice_extents([s.model() for s in srcs], ef, ext, B, n_ext, nbt, zs.room)
        assert mo["status"] == [0] * n_res
        zs.compare(zs.pull(outs), mo, n_res, nbt)
    for resources in (res_a, res_a, res_a, res_b, res_b):
        run(resources, zs.src)
    other = [zs.rig[0].edited(off=hurt), zs.src[1]]
    for srcs in (other, other, zs.src):
        run(res_a, srcs)
    picks = [(0, X3B), (1, 0), (0, 0), (0, ONE)]                  # splice() on a splicer made for extents: n_pick = n_res
    for _ in range(2):
        Splices.check(zs, picks, nbt, splicer=sp)
    sp.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_compress_crc_splice_extents_read_in_one_captured_graph(oracle, fmt):
    """the container's compress and crc, a splice by extents out of it and a reader's read of the new container with checksums, captured
    together -- the splicer's and the reader's first executions inside the capture -- and replayed twice, with other data"""
    import torch
    import ms_compress_amd as m
    import read_model as R
    f, B = FMTS[fmt], 4096
    base = buffers(B)
    resources = [[(0, MIXED, 1, 2)], [(0, X3B, 0, None), (0, X3B5, 0, None)], [], [(0, ZEROS5, 0, 2), (0, TEXT, 2, None)], [(0, ONE, 0, None)]]
    ef, ext = X.flat(resources)
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        rig = Container.make(ctx, f, B, base)
        dev, n = rig.dev, rig.n
        n_res = len(resources)
        lens = [len(b) for b in X.extent_data([base], resources, B)]
        room = sum(lens)
        nbt = n_res + room // B
        sp = m.BlockSplicer.for_extents(ctx, B, 1, n_res, len(ext), nbt)
        d_ef, d_ext = d64(ef, dev), d64(np.array(ext, dtype=np.uint64).reshape(-1), dev)
        d_new = torch.empty(room + 64, dtype=torch.uint8, device=dev)
        d_nfirst, d_noff = torch.zeros(n_res + 1, dtype=torch.int64, device=dev), torch.zeros(nbt + 1, dtype=torch.int64, device=dev)
        d_ncrc, d_nlen = torch.zeros(nbt, dtype=torch.int32, device=dev), torch.zeros(n_res, dtype=torch.int64, device=dev)
        d_st = torch.zeros(n_res, dtype=torch.int32, device=dev)
        reads = [(0, B - 10, 30), (1, 3 * B - 7, 20), (3, 0, ALL), (4, 0, 1), (1, 6 * B, ALL)]
        caps = [30, 20, lens[3], 1, 5]
        ooff, oroom = rig.layout(caps)
        rd = m.BlockReader(ctx, f, B, n_res, nbt, len(reads), 16)
        d_rreq, d_ooff, d_ocap = d64(np.array(reads, dtype=np.uint64).reshape(-1), dev), d64(ooff, dev), d64(caps, dev)
        d_olen, d_ost = torch.zeros(len(reads), dtype=torch.int64, device=dev), torch.zeros(len(reads), dtype=torch.int32, device=dev)
        d_out = torch.empty(oroom, dtype=torch.uint8, device=dev)
        src = (rig.d_packed, rig.d_first, rig.d_boff, rig.d_len, rig.d_crc, rig.total, n, rig.nbt)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rig.compress()
        sp.splice_extents([src], d_ef, d_ext, d_new, d_nfirst, d_noff, d_nlen, d_st, d_new_block_crc=d_ncrc, new_cap=room)
        rd.read(d_new, d_nfirst, d_noff, d_nlen, d_rreq, d_out, d_ooff, d_ocap, d_olen, d_ost, d_block_crc=d_ncrc, packed_len=room)
    for k in range(2):
        bufs = base if k == 0 else [bytes(reversed(b)) for b in base]
        with torch.cuda.stream(s):
            rig.load(bufs)
            d_new.fill_(FILL); d_out.fill_(FILL)
            g.replay()
        s.synchronize()
        data = X.extent_data([bufs], resources, B)
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
def test_res_crc_of_an_extent_container(rigs, fmt, B):
    import torch
    zs = rigs(fmt, B)
    lists = healthy_lists(zs.rig[0].n)
    resources = lists["join"] + lists["insert"] + lists["empties"] + lists["duplicate"] + lists["short_last"]
    n_res, nbt = len(resources), zs.table_for(resources) + 3
    mo, got = zs.check(resources, nbt)
    d_new, d_first, d_off, d_crc, d_len, d_st = got["d"]
    d_rcrc = torch.full((n_res,), 0x33333333, dtype=torch.int32, device=zs.dev)
    d_rst = torch.full((n_res,), ST_FILL, dtype=torch.int32, device=zs.dev)
    zs.m.res_crc_dev(zs.ctx, B, n_res, nbt, d_first, d_len, d_crc, d_rcrc, d_rst)
    zs.ctx.stream.synchronize()
    assert not d_rst.cpu().numpy().any()
    assert [int(x) for x in d_rcrc.cpu().numpy().view(np.uint32)] == [zlib.crc32(b) for b in zs.data(resources)]


def test_host_conveniences(gpu_ctx):
    import ms_compress_amd as m
    f, B = 3, 4096
    bufs0 = buffers(B)
    bufs1 = bufs0[::-1]
    cons = []
    for bufs in (bufs0, bufs1):
        packed, first, off, st = m.blocks_compress(f, bufs, B, ctx=gpu_ctx)
        bcrc, _ = m.blocks_crc(f, bufs, B, ctx=gpu_ctx)
        cons.append((packed, first, off, [len(b) for b in bufs], bcrc))

    def decoded(res, n):
        new_packed, nfirst, noff, nlen, ncrc, status = res
        assert status == [0] * n and ncrc is not None
        out, st = m.blocks_decompress(f, new_packed, nfirst, noff, nlen, B, ctx=gpu_ctx, block_crc=ncrc)
        assert st == [0] * n and [len(o) for o in out] == nlen
        return out
    lists = healthy_lists(len(bufs0))
    resources = lists["join"] + lists["insert"] + lists["empties"]
    assert decoded(m.blocks_splice_extents(cons, resources, B, ctx=gpu_ctx), len(resources)) == X.extent_data([bufs0, bufs1], resources, B)
    assert decoded(m.blocks_concat(cons, [(0, X3B), (1, in1(ZEROS5)), (0, X3B5)], B, ctx=gpu_ctx), 1) == [bufs0[X3B] + bufs0[ZEROS5] + bufs0[X3B5]]
    assert decoded(m.blocks_split_at(cons[0], X3B5, 2, B, ctx=gpu_ctx), 2) == [bufs0[X3B5][: 2 * B], bufs0[X3B5][2 * B:]]
    assert decoded(m.blocks_cut_range(cons[0], MIXED, 1, 2, B, ctx=gpu_ctx), 1) == [bufs0[MIXED][:B] + bufs0[MIXED][3 * B:]]
    plain = m.blocks_splice_extents([c[:4] + (None,) for c in cons], [[(0, X3B, 0, 1)], [(0, BP1, 0, None), (0, X3B, 0, 1)], [(2, 0, 0, None)]], B, ctx=gpu_ctx)
    assert plain[4] is None and plain[5] == [0, M.ARG, M.ARG] and plain[3] == [B, 0, 0]
