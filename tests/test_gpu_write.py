"""GPU: block writers (mscomp_amd_writer_*) against the model of tests/write_model.py -- the whole new packed buffer compared with a sentinel
image (so a byte at or behind new_cap, or behind the container's end, fails), all n_blocks_table + 1 offsets, the whole checksum table,
d_written, d_status, d_res_status and the counts -- on containers made by BlockContainer.compress; and, where every block is healthy,
against a fresh BlockContainer.compress + .crc of the patched data (the header's rule 10)."""
import numpy as np
import pytest

import blocks_model as M
import read_model as R
import write_model as W
from blocks_rig import Container, Writes, d64, flip, long_runs, memo, sources, FMTS, BLOCKS, FILL, ALL, MIXED, TEXT, ZEROS5, MIXED5, RANDOM1

pytestmark = pytest.mark.gpu
ONE, EMPTY = 1, 0                                               # rows of R.RECIPES: the 1-byte resource, an empty one


@pytest.fixture(scope="module")
def rigs(gpu_ctx):
    yield from memo(lambda fmt, B: Writes(Container.make(gpu_ctx, FMTS[fmt], B, R.buffers(B))))


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_geometry(rigs, oracle, fmt, B):
    ws = rigs(fmt, B)
    rig = ws.rig
    L = rig.lens[MIXED]
    reqs = [(MIXED, 0, 10), (MIXED, B // 2, 100), (MIXED, B - 3, 10), (MIXED5, B - 1, B + 2), (MIXED, L - 1, 1), (TEXT, B, B), (ZEROS5, 0, ALL),
            (TEXT, 2 * B + 5, ALL), (MIXED, L + 9, 50), (MIXED, L, ALL), (TEXT, 3 * B + 3, 100), (ONE, 0, 1), (ONE, 0, ALL), (EMPTY, 0, 8), (TEXT, 9, 0),
            (RANDOM1, 0, B), (MIXED5, 3 * B, B)]
    kinds = [1, 2, 1, 2, 1, 1, 2, 0, 1, 1, 1, 1, 2, 1, 1, 0, 1]     # zeros over the raw random block, random bytes over text blocks
    srcs = sources(rig, reqs, 21, kinds)
    for crc in (True, False):
        mo, got = ws.check(oracle, reqs, srcs, crc=crc)
        assert mo["status"] == [0] * len(reqs) and mo["written"] == rig.wants(reqs) and mo["res_status"] == [0] * rig.n
        ws.check_rule_10(got, reqs, srcs)
    j, k = int(rig.first[RANDOM1]), int(rig.first[TEXT]) + 1
    stored = lambda off, b: int(off[b + 1] - off[b])
    assert stored(rig.off, j) == B and stored(mo["off"], j) < B and stored(rig.off, k) < B and stored(mo["off"], k) == B   # the stored form flips both ways


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_every_source_and_destination_residue(rigs, oracle, fmt, B):
    ws = rigs(fmt, B)
    rig = ws.rig
    reqs, res = [], []
    for a in range(16):
        for d in range(16):
            for i, ln in enumerate((1, 15, 16, 17, 4097)):
                r = (MIXED, TEXT)[(a + d + i) % 2]
                reqs.append((r, 16 * ((a * 16 + d) * 7 % 200) + ((a + i) % 2) * B + d, ln))
                res.append(a)
    srcs = sources(rig, reqs, 5, [1] * len(reqs))
    mo, got = ws.check(oracle, reqs, srcs, residues=res)
    assert mo["status"] == [0] * len(reqs)
    ws.check_rule_10(got, reqs, srcs)


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_request_order_decides_overlaps(rigs, oracle, fmt, B):
    ws = rigs(fmt, B)
    rig = ws.rig
    reqs = [(TEXT, 100, 50), (TEXT, 120, 50), (MIXED, 10, 40), (MIXED, 30, 40), (MIXED, 20, 30)]
    # 70 requests into one block -- more units than a wave ranks -- and 70 into another, walking the other way: any order but the request
    # order leaves other bytes
    reqs += [(MIXED5, B + 3 * k, 200) for k in range(70)] + [(ZEROS5, 2 * B + 3 * (69 - k), 200) for k in range(70)]
    srcs = [bytes([q % 251 + 1]) * w for q, w in enumerate(rig.wants(reqs))]
    mo, got = ws.check(oracle, reqs, srcs)
    assert mo["status"] == [0] * len(reqs)
    ws.check_rule_10(got, reqs, srcs)
    pair, bytes_ = [(TEXT, 100, 50), (TEXT, 120, 50)], [b"\x01" * 50, b"\x02" * 50]
    a = ws.check(oracle, pair, bytes_)[1]
    b = ws.check(oracle, pair[::-1], bytes_[::-1])[1]
    assert (a["image"] != b["image"]).any()                          # the same two requests swapped give the other bytes


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_rejects(rigs, oracle, fmt, B):
    ws = rigs(fmt, B)
    rig = ws.rig
    reqs = [(MIXED, 5, 100), (rig.n, 0, 10), (TEXT, B - 1, B + 2), (ALL, 0, 1), (MIXED5, 7, 3 * B), (0, 0, 9), (TEXT, 3 * B, ALL), (RANDOM1, 1, 50)]
    srcs = sources(rig, [q if q[0] < rig.n else (0, 0, 0) for q in reqs], 8)
    assert ws.check(oracle, reqs, srcs, blocks_max=64)[0]["status"] == [0, M.ARG, 0, M.ARG, 0, 0, 0, 0]
    # the budget: covering blocks 1, -, 3, -, 4, 0, 1, 1 -- the requests before the first one past it are applied, those behind it refused
    for bmax, want in ((9, [0, M.ARG, 0, M.ARG, 0, 0, 0, M.ARG]), (8, [0, M.ARG, 0, M.ARG, 0, 0, M.ARG, M.ARG]), (4, [0, M.ARG, 0, M.ARG, M.ARG, 0, M.ARG, M.ARG]),
                       (0, [M.ARG] * 5 + [0, M.ARG, M.ARG])):
        mo, got = ws.check(oracle, reqs, srcs, blocks_max=bmax)
        assert mo["status"] == want, (bmax, mo["status"])
        packed, _, off, crc = rig.fresh(W.patched(rig.bufs, reqs, srcs, [s == 0 for s in want]))
        assert (got["off"] == off).all() and bytes(got["image"][: len(packed)]) == packed and (got["crc"] == crc).all()
    # a resource whose block count is wrong: its requests fail, the others are applied
    bad = rig.first.copy(); bad[MIXED + 1] -= np.uint64(1)
    assert ws.check(oracle, reqs, srcs, first=bad, blocks_max=64)[0]["status"] == [M.DATA, M.ARG, 0, M.ARG, 0, 0, 0, 0]
    # rule 0: the table as a whole
    bad = rig.first.copy(); bad[rig.n] = np.uint64(rig.nbt + 1)
    mo, got = ws.check(oracle, reqs, srcs, first=bad, blocks_max=64)
    assert mo["status"] == [M.ARG] * len(reqs) and mo["res_status"] == [M.ARG] * rig.n and not got["off"].any() and not got["crc"].any()
    bad = rig.first.copy(); bad[2] = bad[3] + np.uint64(1)
    assert ws.check(oracle, reqs, srcs, first=bad, blocks_max=64, crc=False)[0]["status"] == [M.ARG] * len(reqs)
    # no requests: the container is copied unchanged
    for bmax in (0, 4):
        mo, got = ws.check(oracle, [], [], blocks_max=bmax)
        assert mo["packed"] == rig.packed and (got["off"] == rig.off).all() and (got["crc"] == rig.crc).all()


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_damage(rigs, oracle, fmt, B):
    ws = rigs(fmt, B)
    rig = ws.rig
    j = int(rig.first[MIXED])                                     # block 0 raw, block 1 compressed, block 2 raw, block 3 (17 bytes)
    assert int(rig.off[j + 1] - rig.off[j]) == B and int(rig.off[j + 2] - rig.off[j + 1]) < B
    reqs = [(MIXED, 0, 10), (MIXED, B - 1, 2), (MIXED, B + 9, B - 9), (MIXED, 2 * B, 5), (TEXT, 0, ALL), (MIXED, 2 * B - 4, 8), (MIXED, 3 * B, ALL),
            (MIXED + 1, 0, 4 * B)]
    covers = [{0}, {0, 1}, {1}, {2}, set(), {1, 2}, {3}, set()]
    srcs = sources(rig, reqs, 13)
    hit = lambda blocks: [M.DATA if c & blocks else 0 for c in covers]
    # chosen on the CPU so that the model itself refuses: a flipped byte of the raw block and a flipped literal of the compressed one show
    # with checksums only, a broken stream always
    for at, blocks, always in ((int(rig.off[j]) + 77, {0}, False), (flip(oracle, rig, j + 1, B, True), {1}, False), (flip(oracle, rig, j + 1, B, False), {1}, True)):
        hurt = bytearray(rig.packed); hurt[at] ^= 0x01
        d_hurt = rig.d_packed.clone(); d_hurt[at] = int(hurt[at])
        for crc in (True, False):
            mo, got = ws.check(oracle, reqs, srcs, crc=crc, packed=d_hurt, model_packed=bytes(hurt))
            assert mo["status"] == (hit(blocks) if crc or always else [0] * len(reqs))
            if crc or always:                                     # the damaged block is carried verbatim, with its old checksum
                b = j + min(blocks)
                assert int(got["off"][b + 1] - got["off"][b]) == int(rig.off[b + 1] - rig.off[b])
                assert bytes(got["image"][int(got["off"][b]): int(got["off"][b + 1])]) == bytes(hurt[int(rig.off[b]): int(rig.off[b + 1])])
                assert not crc or got["crc"][b] == rig.crc[b]
    # request 5 spans the compressed block 1 (damaged above) and the healthy raw block 2: with 3 refused too, block 2 stays clean
    hurt = bytearray(rig.packed); at = flip(oracle, rig, j + 1, B, False); hurt[at] ^= 0x01
    d_hurt = rig.d_packed.clone(); d_hurt[at] = int(hurt[at])
    few = [reqs[5], reqs[0]]
    mo, got = ws.check(oracle, few, [srcs[5], srcs[0]], packed=d_hurt, model_packed=bytes(hurt))
    assert mo["status"] == [M.DATA, 0] and mo["counts"] == (3, 3, 1)
    assert bytes(got["image"][int(got["off"][j + 2]): int(got["off"][j + 3])]) == rig.packed[int(rig.off[j + 2]): int(rig.off[j + 3])]
    # a clean block with a decreasing table entry gets the stored length 0
    bad = rig.off.copy(); bad[j + 3] = bad[j + 2] - np.uint64(1)
    mo, got = ws.check(oracle, [(TEXT, 0, 4)], [b"abcd"], boff=bad)
    assert mo["status"] == [0] and int(got["off"][j + 3] - got["off"][j + 2]) == 0
    # new_cap one byte short of the need: the last block is absent, its resource refused, the tables complete
    full = ws.check(oracle, reqs, srcs)[0]
    need = int(full["off"][-1])
    mo, got = ws.check(oracle, reqs, srcs, new_cap=need - 1)
    last = max(r for r in range(rig.n) if rig.lens[r])
    assert mo["res_status"] == [M.BUF if r == last else 0 for r in range(rig.n)] and (got["off"] == full["off"]).all()
    assert (got["image"][int(full["off"][int(rig.first[-1]) - 1]):] == FILL).all()


def test_long_runs_and_slice_edges(gpu_ctx, oracle):
    """the move pass where its runs matter, on the container of blocks_rig.long_runs, one writer per case: (a) clean runs longer than 64 rows between
    dirty rows, one of them among hundreds of rows that share a 4096-byte slice; (b) every row behind the first shifted by a constant that
    is no multiple of 16; (c) three raw dirty blocks in consecutive cache slots; (d) as (a), new_cap inside the long resource"""
    rig, g = long_runs(Container, gpu_ctx)
    ws, B, LONG = Writes(rig), rig.B, 1
    stored = lambda off, j: int(off[j + 1] - off[j])
    rs = np.random.RandomState(31)
    # (a) 64 bytes into blocks 0, 70, 200 and 310 (its 17 bytes: the request is clipped)
    a = [(LONG, 100, 64), (LONG, 70 * B + 1000, 64), (LONG, 200 * B + 4000, 64), (LONG, 310 * B, 64)]
    sa = [rs.bytes(64) for _ in a]
    full, got = ws.check(oracle, a, sa)
    assert full["status"] == [0] * 4 and full["written"] == [64, 64, 64, 17] and full["res_status"] == [0] * 3 and full["counts"] == (4, 4, 4)
    assert stored(full["off"], g + 200) != stored(rig.off, g + 200)                 # the rows behind the zero block move
    ws.check_rule_10(got, a, sa)
    # (b) the first small resource's first block changes its stored length
    b, sb = [(0, 33, 64)], [rs.bytes(64)]
    mo, got = ws.check(oracle, b, sb)
    shift = int(mo["off"][g]) - int(rig.off[g])
    assert mo["status"] == [0] and shift % 16 != 0 and (mo["off"][g:] - rig.off[g:] == np.uint64(shift)).all()
    ws.check_rule_10(got, b, sb)
    # (c) 3 B random bytes over blocks 10, 11 and 12: three units in a row, all stored raw
    c, sc = [(LONG, 10 * B, 3 * B)], [rs.bytes(3 * B)]
    mo, got = ws.check(oracle, c, sc)
    assert mo["status"] == [0] and mo["counts"] == (3, 3, 3) and [stored(mo["off"], g + k) for k in (10, 11, 12)] == [B] * 3
    ws.check_rule_10(got, c, sc)
    # (d) new_cap one byte into row 150 of the long resource: that row and everything behind it is absent
    at = int(full["off"][g + 150])
    mo, got = ws.check(oracle, a, sa, new_cap=at + 1)
    assert stored(full["off"], g + 150) > 1 and mo["res_status"] == [0, M.BUF, M.BUF] and mo["status"] == [0] * 4
    assert (got["off"] == full["off"]).all() and len(mo["packed"]) == at and (got["image"][at:] == FILL).all()
    rig.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_repeats_and_ping_pong(rigs, oracle, fmt):
    """one writer executed three times with other requests and other source bytes of the same counts (its graph is captured again when an
    argument moves); then A -> B -> A with further writes, and a reader with the new checksums reads every resource back"""
    B = 4096
    ws = rigs(fmt, B)
    rig = ws.rig
    sets = [[(MIXED, B - 5, 2 * B), (TEXT, 17, 300), (MIXED5, 0, ALL), (0, 0, 5), (MIXED, 0, B)],
            [(MIXED5, 4 * B + 1, ALL), (MIXED, 3 * B, 17), (TEXT, B, B), (TEXT, B + 1, 64), (RANDOM1, 9, 1)],
            [(ZEROS5, 1, 3 * B), (ONE, 0, 1), (TEXT, 0, 1), (MIXED, 2 * B - 1, 2), (MIXED5, 5, 5)]]
    wr = rig.m.BlockWriter(rig.ctx, rig.fmt, B, rig.n, rig.nbt, 5, 12)
    for k in (0, 0, 1, 2, 1):
        srcs = sources(rig, sets[k], 30 + k)
        mo, got = ws.check(oracle, sets[k], srcs, blocks_max=12, writer=wr)
        assert mo["status"] == [0] * 5
    # ping-pong
    s0, s1 = sources(rig, sets[0], 40), sources(rig, sets[1], 41)
    mo0, got0 = ws.check(oracle, sets[0], s0, blocks_max=12, writer=wr)
    d_new, d_noff, d_ncrc = got0["d"]
    plen0 = int(mo0["off"][-1])
    mo1, got1 = ws.check(oracle, sets[1], s1, blocks_max=12, writer=wr, cont=(d_new, plen0, d_noff, d_ncrc),
                         model_cont=(mo0["packed"], plen0, mo0["off"], mo0["crc"]))
    wr.close()
    twice = W.patched(W.patched(rig.bufs, sets[0], s0), sets[1], s1)
    ws.check_rule_10(got1, sets[0] + sets[1], s0 + s1)
    bcrc = got1["crc"]
    got, st = rig.m.blocks_read(rig.fmt, got1["image"][: int(mo1["off"][-1])], rig.first, got1["off"], rig.lens, B, [(r, 0, ALL) for r in range(rig.n)],
                                ctx=rig.ctx, block_crc=bcrc)
    assert st == [0] * rig.n and got == twice


@pytest.mark.parametrize("fmt", list(FMTS))
def test_compress_crc_write_and_read_in_one_captured_graph(oracle, fmt):
    """the container's compress and crc, the writer's write and a reader's read of the new container captured together, the writer's and the
    reader's first executions inside the capture, then replayed with other source bytes written in place between the replays"""
    import torch
    import ms_compress_amd as m
    f, B = FMTS[fmt], 4096
    base = R.buffers(B)
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        rig = Container.make(ctx, f, B, base)
        dev = rig.dev
        reqs = [(MIXED, B - 5, 2 * B), (TEXT, 17, 300), (MIXED5, 0, ALL), (0, 0, 5), (MIXED, 0, B), (RANDOM1, 0, ALL), (TEXT, 2 * B + 9, ALL)]
        wants = rig.wants(reqs)
        soff, sroom = rig.layout(wants)
        wr = m.BlockWriter(ctx, f, B, rig.n, rig.nbt, len(reqs), 24)
        d_req, d_soff = d64(np.array(reqs, dtype=np.uint64).reshape(-1), dev), d64(soff, dev)
        d_src = torch.zeros(sroom, dtype=torch.uint8, device=dev)
        d_new = torch.empty(rig.total + 64, dtype=torch.uint8, device=dev)
        d_noff, d_ncrc = torch.zeros(rig.nbt + 1, dtype=torch.int64, device=dev), torch.zeros(max(1, rig.nbt), dtype=torch.int32, device=dev)
        d_wr, d_st = torch.zeros(len(reqs), dtype=torch.int64, device=dev), torch.zeros(len(reqs), dtype=torch.int32, device=dev)
        d_rst = torch.zeros(rig.n, dtype=torch.int32, device=dev)
        reads = [(r, 0, ALL) for r in range(rig.n)]
        ooff, oroom = rig.layout(rig.lens)
        rd = m.BlockReader(ctx, f, B, rig.n, rig.nbt, rig.n, int(rig.first[-1]))
        d_rreq, d_ooff, d_ocap = d64(np.array(reads, dtype=np.uint64).reshape(-1), dev), d64(ooff, dev), d64(rig.lens, dev)
        d_olen, d_ost = torch.zeros(rig.n, dtype=torch.int64, device=dev), torch.zeros(rig.n, dtype=torch.int32, device=dev)
        d_out = torch.empty(oroom, dtype=torch.uint8, device=dev)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rig.compress()
        wr.write(rig.d_packed, rig.d_first, rig.d_boff, rig.d_len, d_req, d_src, d_soff, d_new, d_noff, d_wr, d_st, d_rst, d_block_crc=rig.d_crc,
                 d_new_block_crc=d_ncrc, packed_len=rig.total, new_cap=rig.total)
        rd.read(d_new, rig.d_first, d_noff, rig.d_len, d_rreq, d_out, d_ooff, d_ocap, d_olen, d_ost, d_block_crc=d_ncrc, packed_len=rig.total)
    for k in range(2):
        srcs = sources(rig, reqs, 50 + k, [(q + k) % 3 for q in range(len(reqs))])
        blob = np.zeros(sroom, dtype=np.uint8)
        for o, sb in zip(soff, srcs):
            blob[o: o + len(sb)] = np.frombuffer(sb, dtype=np.uint8)
        with torch.cuda.stream(s):
            d_src.copy_(torch.from_numpy(blob))
            d_new.fill_(FILL); d_out.fill_(FILL)
            g.replay()
        s.synchronize()
        want = W.patched(base, reqs, srcs)
        assert not d_st.cpu().numpy().any() and not d_rst.cpu().numpy().any() and not d_ost.cpu().numpy().any(), k
        assert [int(x) for x in d_wr.cpu().numpy()] == wants
        out = d_out.cpu().numpy()
        image = np.full(oroom, FILL, dtype=np.uint8)
        for o, b in zip(ooff, want):
            image[o: o + len(b)] = np.frombuffer(b, dtype=np.uint8)
        assert (out == image).all(), k
        total = sum(rig.lens)
        packed, _, off, _ = M.model_compress(oracle, f, want, B, total, total)
        assert (d_noff.cpu().numpy().view(np.uint64) == off).all() and bytes(d_new.cpu().numpy()[: len(packed)]) == packed
        assert (d_new.cpu().numpy()[len(packed):] == FILL).all()
        assert (d_ncrc.cpu().numpy().view(np.uint32)[: rig.nbt] == R.block_crcs(want, B, rig.nbt)).all()
    del g
    rd.close(); wr.close()
    rig.close()
    ctx.close()


def test_host_convenience(gpu_ctx, oracle):
    import ms_compress_amd as m
    f, B = 3, 4096
    bufs = R.buffers(B)
    lens = [len(b) for b in bufs]
    total = sum(lens)
    packed, first, off, st = m.blocks_compress(f, bufs, B, ctx=gpu_ctx)
    bcrc, _ = m.blocks_crc(f, bufs, B, ctx=gpu_ctx)
    nbt = len(off) - 1
    writes = [(MIXED, B - 5, bytes(2 * B)), (TEXT, 17, b"x" * 300), (len(bufs), 0, b"y"), (MIXED, 3 * B + 10, b"0123456789"), (MIXED, 7, b""), (ZEROS5, 1, b"\x07" * 9)]
    reqs, srcs = [(r, o, len(b)) for r, o, b in writes], [b for _, _, b in writes]
    for crc in (None, bcrc):
        mo = W.model_write(oracle, f, bytes(packed), len(packed), first, off, lens, B, nbt, reqs, srcs, 1 << 30, total, crc)
        new_packed, noff, ncrc, written, status, res_status = m.blocks_write(f, packed, first, off, lens, B, writes, ctx=gpu_ctx, block_crc=crc)
        assert status == mo["status"] == [0, 0, M.ARG, 0, 0, 0] and written == mo["written"] == [2 * B, 300, 0, 7, 0, 9] and res_status == [0] * len(bufs)
        assert bytes(new_packed) == mo["packed"] and (noff == mo["off"]).all()
        assert (ncrc is None) if crc is None else (ncrc == mo["crc"]).all()
