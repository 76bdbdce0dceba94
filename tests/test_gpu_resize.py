"""GPU: mscomp_amd_writer_resize against the model of tests/resize_model.py -- the whole new packed buffer compared with a sentinel image (so a
byte at or behind new_cap, or behind the container's end, fails), every entry of the four new tables, d_res_status and the counts -- on the
container of tests/blocks_rig.Container with a table of 16 spare rows and blocks_max = 24; where the container is healthy also byte for byte
against BlockContainer.compress + .crc of the resized data, and every new container is read back. mscomp_amd_res_crc_dev against zlib.crc32."""
import zlib

import numpy as np
import pytest

import blocks_model as M
import read_model as R
import resize_model as Z
import write_model as W
from blocks_rig import Container, Resizes, d64, long_runs, memo, BUDGET, FMTS, BLOCKS, FILL, ALL, MIXED, TEXT, ZEROS5, MIXED5
from resize_model import SPARE, mixes

pytestmark = pytest.mark.gpu


def _counts(lens, want, B):
    """(units, changed blocks, blocks encoded) of a call that accepts every resource"""
    geo = [Z.geometry(L, x, (L + B - 1) // B, B) for L, x in zip(lens, want) if L != x]
    return (sum(c for _, _, c in geo), sum(1 for _, ch, _ in geo if ch), sum(c for _, _, c in geo))


@pytest.fixture(scope="module")
def rigs(gpu_ctx):
    yield from memo(lambda fmt, B: Resizes(Container.make(gpu_ctx, FMTS[fmt], B, R.buffers(B))))


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_geometry(rigs, oracle, fmt, B):
    """per resource every wanted length of resize_model.WANTS -- cuts inside the tail block, inside a full block and at a boundary,
    extension of a partial and of an aligned tail and of an empty resource, truncation to nothing --, mixed in one call"""
    zs = rigs(fmt, B)
    rig = zs.rig
    for v, want in enumerate(mixes(rig.lens, B)):
        for crc in ((True, False) if v == 0 else (True,)):
            mo, got = zs.check(oracle, want, crc=crc)
            assert mo["res_status"] == [0] * rig.n and mo["new_len"] == want, v
            data = Z.resized(rig.bufs, want)
            zs.check_consequence(got, data)
            if crc:                                               # the resource checksums, from the new block checksums alone
                d_new, d_nfirst, d_noff, d_ncrc, d_nlen, _ = got["d"]
                assert zs.res_crc(d_nfirst, d_nlen, d_ncrc) == ([zlib.crc32(b) for b in data], [0] * rig.n)
    # a cut exactly at a block boundary has no changed block and decodes nothing; W = 0 drops everything
    want = list(rig.lens); want[MIXED] = 2 * B; want[MIXED5] = 0; want[TEXT] = 3 * B
    assert zs.check(oracle, want)[0]["counts"] == (0, 0, 0)


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_renumbering(rigs, oracle, fmt, B):
    zs = rigs(fmt, B)
    rig = zs.rig
    nb = int(rig.first[-1])
    want = list(rig.lens); want[0] = 5 * B                       # the first resource grows by 5 blocks in front of 11 untouched ones
    mo, got = zs.check(oracle, want)
    assert mo["counts"] == (5, 0, 5) and (got["first"][1:] == rig.first[1:] + np.uint64(5)).all()
    at = int(got["off"][5])
    assert bytes(got["image"][at: at + rig.plen]) == rig.packed and (got["off"][5: 5 + nb + 1] - np.uint64(at) == rig.off[: nb + 1]).all()
    assert (got["crc"][5: 5 + nb] == rig.crc[:nb]).all()
    zs.check_consequence(got, Z.resized(rig.bufs, want))
    want = list(rig.lens); want[ZEROS5] = B                       # one shrinks by 4: nothing is decoded or encoded, the rows behind it move up
    mo, got = zs.check(oracle, want)
    j = int(rig.first[ZEROS5])
    assert mo["counts"] == (0, 0, 0) and (got["first"][ZEROS5 + 1:] == rig.first[ZEROS5 + 1:] - np.uint64(4)).all()
    assert (got["crc"][: j + 1] == rig.crc[: j + 1]).all() and (got["crc"][j + 1: nb - 4] == rig.crc[j + 5: nb]).all()
    assert bytes(got["image"][: int(got["off"][nb - 4])]) == rig.packed[: int(rig.off[j + 1])] + rig.packed[int(rig.off[j + 5]):]
    zs.check_consequence(got, Z.resized(rig.bufs, want))


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_rejects(rigs, oracle, fmt, B):
    zs = rigs(fmt, B)
    rig = zs.rig
    n, lens = rig.n, rig.lens
    grow = [L + 1 for L in lens]
    # rule 0, both forms: MSCOMP_ARG_ERROR and zeros only
    beyond = rig.first.copy(); beyond[n] = np.uint64(zs.nbt + 1)
    falling = rig.first.copy(); falling[3] = falling[4] + np.uint64(1)
    for bad, crc in ((beyond, True), (falling, True), (falling, False)):
        mo, got = zs.check(oracle, grow, first=bad, crc=crc)
        assert mo["res_status"] == [M.ARG] * n and not got["first"].any() and not got["off"].any() and not any(got["new_len"]) and mo["counts"] == (0, 0, 0)
        assert (got["image"] == FILL).all() and (crc is False or not got["crc"].any())
    # rule 1: a length that asks for one block more than the table has; the resource is carried with the blocks it has
    odd = list(lens); odd[MIXED] += B
    want = list(lens); want[MIXED] = 5; want[TEXT] = lens[TEXT] + B
    mo, got = zs.check(oracle, want, lens=odd, read_back=False)
    assert mo["res_status"] == [M.DATA if r == MIXED else 0 for r in range(n)] and mo["new_len"][MIXED] == odd[MIXED]
    # rule 3: costs 1, 2, 3, 1 and a free cut; the third changing resource crosses a budget of 3, and everything that changes behind it is
    # refused too, the cheaper ones and the free cut included: the sum includes refused ones
    want = list(lens); want[2] = lens[2] - 1; want[4] = 2 * B + 1; want[MIXED] = lens[MIXED] + 3 * B - 17; want[TEXT] = lens[TEXT] - 1; want[9] = 2 * B
    for bmax, st in ((7, {}), (6, {TEXT: M.ARG, 9: M.ARG}), (3, {MIXED: M.ARG, TEXT: M.ARG, 9: M.ARG}), (0, {2: M.ARG, 4: M.ARG, MIXED: M.ARG, TEXT: M.ARG, 9: M.ARG})):
        mo, got = zs.check(oracle, want, blocks_max=bmax)
        assert mo["res_status"] == [st.get(r, 0) for r in range(n)], bmax
        zs.check_consequence(got, Z.resized(rig.bufs, mo["new_len"]))
    # rule 8: a table one row short is refused as a whole; the same growth less one block fills the table to its last row
    want = list(lens); want[0] = (SPARE + 1) * B
    mo, got = zs.check(oracle, want)
    assert mo["res_status"] == [M.ARG] * n and not got["first"].any() and not got["off"].any() and mo["counts"] == (0, 0, 0) and (got["image"] == FILL).all()
    want[0] = SPARE * B
    mo, got = zs.check(oracle, want)
    assert mo["res_status"] == [0] * n and int(got["first"][-1]) == zs.nbt
    zs.check_consequence(got, Z.resized(rig.bufs, want))
    # rule 10: new_cap cuts inside the first dirty block, and inside a carried block; MSCOMP_BUF_ERROR replaces the other status
    want = list(lens); want[2] = lens[2] - 100
    full = zs.check(oracle, want)[0]
    d = int(full["first"][2])
    mo, got = zs.check(oracle, want, new_cap=int(full["off"][d + 1]) - 1)
    assert mo["res_status"] == [0, 0] + [M.BUF] * 9 + [0] and (got["off"] == full["off"]).all() and (got["image"][int(full["off"][d]):] == FILL).all()
    full = zs.check(oracle, want, lens=odd, read_back=False)[0]
    g = int(full["first"][MIXED])
    mo, got = zs.check(oracle, want, lens=odd, new_cap=int(full["off"][g + 2]) - 1, read_back=False)
    assert full["res_status"][MIXED] == M.DATA and mo["res_status"][MIXED] == M.BUF and mo["res_status"][:MIXED] == [0] * MIXED


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_damage(rigs, oracle, fmt, B):
    zs = rigs(fmt, B)
    rig = zs.rig
    n, lens = rig.n, rig.lens
    j = int(rig.first[MIXED])                                     # block 0 raw, block 1 compressed, block 2 raw, block 3 (17 bytes)
    assert int(rig.off[j + 1] - rig.off[j]) == B and int(rig.off[j + 3] - rig.off[j + 2]) == B
    at = int(rig.off[j]) + 77
    hurt = bytearray(rig.packed); hurt[at] ^= 0x01
    d_hurt = rig.d_packed.clone(); d_hurt[at] = int(hurt[at])
    want = list(lens); want[MIXED] = 5 * B + 100; want[MIXED - 1] = 3 * B; want[MIXED + 1] = 0
    # the cut falls into healthy block 3 while damaged block 0 is clean: carried verbatim, nobody looks
    assert zs.check(oracle, want, packed=d_hurt, model_packed=bytes(hurt))[0]["res_status"] == [0] * n
    # the changed block is the damaged one: with checksums the resource is carried -- its fresh blocks absent, its neighbours resized --,
    # without them the flip in a raw block is accepted silently, as the writer does
    want[MIXED] = 100
    mo, got = zs.check(oracle, want, packed=d_hurt, model_packed=bytes(hurt))
    assert mo["res_status"] == [M.DATA if r == MIXED else 0 for r in range(n)] and mo["new_len"][MIXED] == lens[MIXED] and mo["counts"] == (3, 2, 2)
    g = int(got["first"][MIXED])
    assert int(got["first"][MIXED + 1]) == g + 4 and (got["crc"][g: g + 4] == rig.crc[j: j + 4]).all()
    assert bytes(got["image"][int(got["off"][g]): int(got["off"][g + 4])]) == bytes(hurt)[int(rig.off[j]): int(rig.off[j + 4])]
    mo, got = zs.check(oracle, want, crc=False, packed=d_hurt, model_packed=bytes(hurt))
    assert mo["res_status"] == [0] * n and mo["new_len"] == want
    # an unreadable clean entry becomes an empty one
    bad = zs.off.copy(); bad[j + 3] = bad[j + 2] - np.uint64(1)
    want = list(lens); want[TEXT] = 9
    mo, got = zs.check(oracle, want, boff=bad)
    assert mo["res_status"] == [0] * n and int(got["off"][j + 3] - got["off"][j + 2]) == 0
    # rule 8 on the final counts: a growth of SPARE + 1 rows fits because a cut frees one -- unless the cut's changed block is unreadable,
    # so that the cut is carried and counts with the rows it had
    want = list(lens); want[0] = (SPARE + 1) * B; want[MIXED] = lens[MIXED] - 18
    assert zs.check(oracle, want)[0]["res_status"] == [0] * n
    at = int(rig.off[j + 2]) + 7
    hurt = bytearray(rig.packed); hurt[at] ^= 0x55
    d_hurt = rig.d_packed.clone(); d_hurt[at] = int(hurt[at])
    mo, got = zs.check(oracle, want, packed=d_hurt, model_packed=bytes(hurt))
    assert mo["res_status"] == [M.ARG] * n and not got["off"].any() and mo["counts"] == (0, 0, 0)


def test_long_runs_and_slice_edges(gpu_ctx, oracle):
    """the move pass where its runs matter, on the container of blocks_rig.long_runs: (a) 311 clean rows in one run that is shifted by
    a row as well as by bytes; (b) a clean run that ends at its resource's changed block, the resource behind it a run at another distance;
    (c) the long resource carried with MSCOMP_DATA_ERROR between two that change; (d) as (b), new_cap inside the long resource"""
    rig, g = long_runs(Container, gpu_ctx)
    zs, B, lens = Resizes(rig), rig.B, rig.lens
    # (a) the first cut to 1 byte, the last extended by 2 B + 5
    want = [1, lens[1], lens[2] + 2 * B + 5]
    mo, got = zs.check(oracle, want)
    g2 = int(got["first"][1])
    assert mo["res_status"] == [0] * 3 and mo["new_len"] == want and g2 == g - 1 and (int(got["off"][g2]) - int(rig.off[g])) % 16 != 0
    assert (got["off"][g2: g2 + 312] - got["off"][g2] == rig.off[g: g + 312] - rig.off[g]).all()
    zs.check_consequence(got, Z.resized(rig.bufs, want))
    # (b) the long one cut by 100 B + 7: 211 blocks, the last one changed
    want = [lens[0], lens[1] - (100 * B + 7), lens[2]]
    full, got = zs.check(oracle, want)
    assert full["res_status"] == [0] * 3 and full["new_len"] == want and full["counts"] == (1, 1, 1) and int(got["first"][2]) == g + 211
    assert int(got["off"][g + 211]) - int(rig.off[g + 311]) != int(got["off"][g + 210]) - int(rig.off[g + 210])
    zs.check_consequence(got, Z.resized(rig.bufs, want))
    # (c) a length that asks for one block more than the long resource has
    odd = list(lens); odd[1] += B
    want = [1, lens[1] - 5, lens[2] + 2 * B + 5]
    mo, got = zs.check(oracle, want, lens=odd, read_back=False)
    assert mo["res_status"] == [0, M.DATA, 0] and mo["new_len"] == [1, odd[1], want[2]] and int(got["first"][2]) - int(got["first"][1]) == 311
    # (d) new_cap one byte into row 100 of the long resource
    want = [lens[0], lens[1] - (100 * B + 7), lens[2]]
    at = int(full["off"][g + 100])
    mo, got = zs.check(oracle, want, new_cap=at + 1)
    assert int(full["off"][g + 101]) - at > 1 and mo["res_status"] == [0, M.BUF, M.BUF] and (got["off"] == full["off"]).all()
    assert len(mo["packed"]) == at and (got["image"][at:] == FILL).all()
    zs.close()


def test_checksum_arrays_come_in_pairs(rigs):
    import torch
    zs = rigs("xpress", 4096)
    rig = zs.rig
    d_new, d_nfirst, d_noff, d_ncrc, d_nlen, d_rst = zs.outputs()
    wr = rig.m.BlockWriter(rig.ctx, rig.fmt, rig.B, rig.n, zs.nbt, 0, BUDGET)
    for old, new in ((zs.d_crc, None), (None, d_ncrc)):
        with pytest.raises(rig.m.MSCompError) as e:
            wr.resize(rig.d_packed, rig.d_first, zs.d_boff, rig.d_len, rig.d_len, d_new, d_nfirst, d_noff, d_nlen, d_rst, d_block_crc=old, d_new_block_crc=new,
                      packed_len=rig.plen)
        assert e.value.status == rig.m.MSCOMP_ARG_ERROR
    wr.close()
    torch.cuda.synchronize()
    assert (d_new.cpu().numpy() == FILL).all()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_repeats_and_ping_pong(rigs, oracle, fmt):
    """one writer: resize A -> B, write into the grown region B -> A, resize back A -> B, each step five times (its graph replayed from the
    second execution on; write and resize keep graphs of their own); the final container is compress of the final data"""
    import torch
    B = 4096
    zs = rigs(fmt, B)
    rig, dev = zs.rig, zs.rig.dev
    L = rig.lens[MIXED]
    want1 = list(rig.lens); want1[MIXED] = L + 2 * B + 5; want1[TEXT] = B + 7; want1[0] = 100
    reqs = [(MIXED, L - 3, 2 * B + 8), (0, 10, 50)]
    srcs = [np.random.RandomState(77).bytes(2 * B + 8), (b"grown " * 9)[:50]]
    wants = [len(s) for s in srcs]
    soff, sroom = rig.layout(wants)
    blob = np.zeros(sroom, dtype=np.uint8)
    for o, s in zip(soff, srcs):
        blob[o: o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    d_src, d_soff, d_req = torch.from_numpy(blob).to(dev), d64(soff, dev), d64(np.array(reqs, dtype=np.uint64).reshape(-1), dev)
    d_wr, d_st = torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    d_rst = torch.zeros(rig.n, dtype=torch.int32, device=dev)
    wr = rig.m.BlockWriter(rig.ctx, rig.fmt, B, rig.n, zs.nbt, 2, BUDGET)
    b_new, b_first, b_off, b_crc, b_len, b_rst = zs.outputs()
    a_new, _, a_off, a_crc, _, _ = zs.outputs()
    c_new, c_first, c_off, c_crc, c_len, c_rst = zs.outputs()
    d_want1 = d64(want1, dev)
    for _ in range(5):
        wr.resize(rig.d_packed, rig.d_first, zs.d_boff, rig.d_len, d_want1, b_new, b_first, b_off, b_len, b_rst, d_block_crc=zs.d_crc, d_new_block_crc=b_crc,
                  packed_len=rig.plen, new_cap=zs.room)
    assert wr.counts() == _counts(rig.lens, want1, B) and not b_rst.cpu().numpy().any()
    for _ in range(5):
        wr.write(b_new, b_first, b_off, b_len, d_req, d_src, d_soff, a_new, a_off, d_wr, d_st, d_rst, d_block_crc=b_crc, d_new_block_crc=a_crc,
                 packed_len=zs.room, new_cap=zs.room)
    assert not d_st.cpu().numpy().any() and not d_rst.cpu().numpy().any() and [int(x) for x in d_wr.cpu().numpy()] == wants
    d_want2 = d64(rig.lens, dev)
    for _ in range(5):
        wr.resize(a_new, b_first, a_off, b_len, d_want2, c_new, c_first, c_off, c_len, c_rst, d_block_crc=a_crc, d_new_block_crc=c_crc, packed_len=zs.room,
                  new_cap=zs.room)
    counts = wr.counts()
    wr.close()
    assert not c_rst.cpu().numpy().any() and [int(x) for x in c_len.cpu().numpy()] == rig.lens and counts == _counts(want1, rig.lens, B)
    final = Z.resized(W.patched(Z.resized(rig.bufs, want1), reqs, srcs), rig.lens)
    got = {"image": c_new.cpu().numpy(), "first": c_first.cpu().numpy().view(np.uint64), "off": c_off.cpu().numpy().view(np.uint64),
           "crc": c_crc.cpu().numpy().view(np.uint32)}
    zs.check_consequence(got, final)
    assert (got["image"][int(got["off"][-1]):] == FILL).all()
    zs.read_back(got, final)


@pytest.mark.parametrize("fmt", list(FMTS))
def test_compress_crc_resize_res_crc_and_read_in_one_captured_graph(oracle, fmt):
    """the container's compress and crc, the writer's resize, mscomp_amd_res_crc_dev and a reader's read of a range that straddles the old
    end, captured together -- the writer's and the reader's first executions inside the capture -- and replayed twice, with other data"""
    import torch
    import ms_compress_amd as m
    f, B = FMTS[fmt], 4096
    base = R.buffers(B)
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        rig = Container.make(ctx, f, B, base)
        dev, n, nbt = rig.dev, rig.n, rig.nbt
        L = rig.lens[MIXED]
        want = list(rig.lens); want[MIXED] = L + B + 9; want[TEXT] = B + 3; want[0] = 2 * B
        room = rig.total + 4 * B
        wr = m.BlockWriter(ctx, f, B, n, nbt, 0, 8)
        d_want = d64(want, dev)
        d_new = torch.empty(room + 64, dtype=torch.uint8, device=dev)
        d_nfirst, d_noff = torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(nbt + 1, dtype=torch.int64, device=dev)
        d_ncrc, d_nlen = torch.zeros(nbt, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
        d_rst, d_rcrc, d_cst = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
        reads = [(MIXED, L - 10, 30), (TEXT, 0, ALL), (0, B - 1, 2), (MIXED5, 0, ALL)]
        caps = [30, B + 3, 2, 5 * B]
        ooff, oroom = rig.layout(caps)
        rd = m.BlockReader(ctx, f, B, n, nbt, len(reads), 16)
        d_rreq, d_ooff, d_ocap = d64(np.array(reads, dtype=np.uint64).reshape(-1), dev), d64(ooff, dev), d64(caps, dev)
        d_olen, d_ost = torch.zeros(len(reads), dtype=torch.int64, device=dev), torch.zeros(len(reads), dtype=torch.int32, device=dev)
        d_out = torch.empty(oroom, dtype=torch.uint8, device=dev)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rig.compress()
        wr.resize(rig.d_packed, rig.d_first, rig.d_boff, rig.d_len, d_want, d_new, d_nfirst, d_noff, d_nlen, d_rst, d_block_crc=rig.d_crc, d_new_block_crc=d_ncrc,
                  packed_len=rig.total, new_cap=room)
        m.res_crc_dev(ctx, B, n, nbt, d_nfirst, d_nlen, d_ncrc, d_rcrc, d_cst)
        rd.read(d_new, d_nfirst, d_noff, d_nlen, d_rreq, d_out, d_ooff, d_ocap, d_olen, d_ost, d_block_crc=d_ncrc, packed_len=room)
    for k in range(2):
        bufs = base if k == 0 else [bytes(reversed(b)) for b in base]
        with torch.cuda.stream(s):
            rig.load(bufs)
            d_new.fill_(FILL); d_out.fill_(FILL)
            g.replay()
        s.synchronize()
        data = Z.resized(bufs, want)
        assert not d_rst.cpu().numpy().any() and not d_cst.cpu().numpy().any() and not d_ost.cpu().numpy().any(), k
        assert [int(x) for x in d_nlen.cpu().numpy()] == want
        assert [int(x) for x in d_rcrc.cpu().numpy().view(np.uint32)] == [zlib.crc32(b) for b in data]
        image = np.full(oroom, FILL, dtype=np.uint8)
        for o, (r, at, ln), c in zip(ooff, reads, caps):
            image[o: o + c] = np.frombuffer(data[r][at: at + c], dtype=np.uint8)
        assert (d_out.cpu().numpy() == image).all(), k
        total = sum(want)
        packed, first, off, _ = M.model_compress(oracle, f, data, B, total, total)
        nb = int(first[-1])
        assert (d_nfirst.cpu().numpy().view(np.uint64) == first).all() and (d_noff.cpu().numpy().view(np.uint64)[: nb + 1] == off[: nb + 1]).all()
        assert bytes(d_new.cpu().numpy()[: len(packed)]) == packed and (d_new.cpu().numpy()[len(packed):] == FILL).all()
        assert (d_ncrc.cpu().numpy().view(np.uint32) == R.block_crcs(data, B, nbt)).all()
    del g
    rd.close(); wr.close()
    rig.close()
    ctx.close()


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_res_crc(rigs, oracle, fmt, B):
    import torch
    zs = rigs(fmt, B)
    rig = zs.rig
    n, lens = rig.n, rig.lens
    want = [zlib.crc32(b) for b in rig.bufs]
    assert zs.res_crc(rig.d_first, rig.d_len, zs.d_crc) == (want, [0] * n)
    d_bcrc, d_rcrc = torch.zeros(max(1, rig.nbt), dtype=torch.int32, device=rig.dev), torch.zeros(n, dtype=torch.int32, device=rig.dev)
    rig.bk.crc(rig.d_in, rig.d_off, rig.d_len, d_bcrc, rig.d_cst, d_res_crc=d_rcrc)    # what mscomp_amd_blocks_crc says of the same resources
    rig.ctx.stream.synchronize()
    assert [int(x) for x in d_rcrc.cpu().numpy().view(np.uint32)] == want
    # the rejects: a wrong count (here and in the next resource), a table entry beyond the table
    bad = rig.first.copy(); bad[MIXED + 1] -= np.uint64(1)
    got = zs.res_crc(d64(bad, rig.dev), rig.d_len, zs.d_crc)
    mo = Z.model_res_crc(bad, lens, zs.crc, B, zs.nbt)
    assert got == ([int(x) for x in mo[0]], mo[1]) and got[1][MIXED] == got[1][MIXED + 1] == M.DATA and got[0][MIXED] == 0
    bad = rig.first.copy(); bad[n] = np.uint64(zs.nbt + 1)
    got = zs.res_crc(d64(bad, rig.dev), rig.d_len, zs.d_crc)
    mo = Z.model_res_crc(bad, lens, zs.crc, B, zs.nbt)
    assert got == ([int(x) for x in mo[0]], mo[1]) and got[1][n - 1] == M.ARG


def test_res_crc_after_a_write(gpu_ctx, oracle):
    import ms_compress_amd as m
    f, B = 4, 4096
    bufs = R.buffers(B)
    lens = [len(b) for b in bufs]
    packed, first, off, st = m.blocks_compress(f, bufs, B, ctx=gpu_ctx)
    bcrc, rcrc = m.blocks_crc(f, bufs, B, ctx=gpu_ctx)
    writes = [(MIXED, B - 5, bytes(2 * B)), (TEXT, 17, b"x" * 300), (ZEROS5, 1, b"\x07" * 9)]
    _, _, ncrc, _, status, _ = m.blocks_write(f, packed, first, off, lens, B, writes, ctx=gpu_ctx, block_crc=bcrc)
    new = W.patched(bufs, [(r, o, len(b)) for r, o, b in writes], [b for _, _, b in writes])
    got, st = m.res_crc_from_blocks(first, lens, ncrc, B, ctx=gpu_ctx)
    assert status == [0] * 3 and st == [0] * len(bufs) and [int(x) for x in got] == [zlib.crc32(b) for b in new]
    assert [int(x) for x in got] != [int(x) for x in rcrc]           # (the checksums blocks_crc once wrote are stale)


def test_res_crc_one_resource_of_3000_blocks(gpu_ctx):
    import ms_compress_amd as m
    B, nblk = 4096, 3000
    data = np.random.RandomState(3000).bytes(nblk * B - 5)
    bcrc = R.block_crcs([b"", data, b"tail"], B, nblk + 9)          # block checksums of generated data: nothing is compressed or decoded
    first = np.array([0, 0, nblk, nblk + 1], dtype=np.uint64)
    got, st = m.res_crc_from_blocks(first, [0, len(data), 4], bcrc, B, ctx=gpu_ctx)
    assert st == [0, 0, 0] and [int(x) for x in got] == [0, zlib.crc32(data), zlib.crc32(b"tail")]


def test_host_convenience(gpu_ctx, oracle):
    import ms_compress_amd as m
    f, B = 3, 4096
    bufs = R.buffers(B)
    lens = [len(b) for b in bufs]
    packed, first, off, st = m.blocks_compress(f, bufs, B, ctx=gpu_ctx)
    bcrc, _ = m.blocks_crc(f, bufs, B, ctx=gpu_ctx)
    want = list(lens); want[0] = 3 * B + 1; want[MIXED] = B + 9; want[ZEROS5] = 0; want[TEXT] = lens[TEXT] + 5
    data = Z.resized(bufs, want)
    total = sum(want)
    for crc in (None, bcrc):
        new_packed, noff, ncrc, nfirst, nlen, status = m.blocks_resize(f, packed, first, off, lens, B, want, ctx=gpu_ctx, block_crc=crc)
        mp, mf, mo, _ = M.model_compress(oracle, f, data, B, total, total)
        nb = int(mf[-1])
        assert status == [0] * len(bufs) and nlen == want and (nfirst == mf).all() and (noff == mo[: nb + 1]).all() and bytes(new_packed) == mp
        assert (ncrc is None) if crc is None else (ncrc == R.block_crcs(data, B, nb)).all()
    got, st = m.res_crc_from_blocks(nfirst, nlen, ncrc, B, ctx=gpu_ctx)
    assert st == [0] * len(bufs) and [int(x) for x in got] == [zlib.crc32(b) for b in data]
