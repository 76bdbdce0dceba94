"""GPU: every block object on containers whose stored bytes lie at offsets that need more than 31 and more than 32 bits (tests/far_rig.py:
one arena of 4 GiB + 64 MiB, of which a case writes a few small windows; blocks_rig.Container.far). The store is sync_model.store_buffers:
3 B + 17 mixed bytes (raw and compressed blocks, a short last one), 5 B zeros, one raw block -- made once per format at B = 4096 with
Container.make; the far copies come from it. One B = 65536 Xpress+Huffman store serves the container, reader and transcoder cases.

Each object runs the plain case of its rig -- and one refused resource where the rig has one -- through the rig's own check, so every
output is compared with the object's model (which reads a FarBytes: nothing in front of the container); then the same call on the near
container must give the same outputs, the input-side offsets apart. Where an object also takes offsets of plain bytes (d_res_off,
d_out_off, the reader's output offsets, the writer's source offsets, the syncer's unit offsets), those lie in a second far window at
another place. The aliases of a container's window hold a decoy: its stored bytes with one byte of every block changed so that the block
still decodes where such a byte exists -- a cut offset reads a valid container with other contents."""
import copy
import zlib

import numpy as np
import pytest

import blocks_model as M
import crc_model as K
import diff_model as F
import digest_model as G
import sync_model as Y
import far_rig as FR
from blocks_rig import (Container, Extents, ReadRig, Resizes, Splices, Spliced, Writes, check_dedup, d64, memo, odd_offsets, same_image, sources,
                        CRC_FILL, FILL, FMTS, SENT32, ST_FILL)
from parity_rig import FixOuts, check_build, check_rebuild, lose
from repair_rig import check_repair, check_salvage, rebuild as repair_rebuild
from test_gpu_diff import check_diff, rebuild as diff_rebuild
from test_gpu_digest import DRig, digests_of
from test_gpu_match import check_match, rebuild as match_rebuild
from test_gpu_transcode import Run, Source, same as same_transcode

pytestmark = pytest.mark.gpu
B = 4096
SHAPES = [(f, B, b) for f in FMTS for b in FR.BASES]
WIDE = [("xpress_huff", 65536, b) for b in FR.BASES]            # the container, reader and transcoder cases only
shapes = pytest.mark.parametrize("fmt,B,base", SHAPES)
shapes_wide = pytest.mark.parametrize("fmt,B,base", SHAPES + WIDE)


@pytest.fixture(scope="module")
def made(gpu_ctx):
    """near containers by name, made once"""
    yield from memo()


def the_store(ctx, made, fmt, B, order=(0, 1, 2), name="store"):
    bufs = Y.store_buffers(B)
    return made((fmt, B, name), lambda: ReadRig.make(ctx, FMTS[fmt], B, [bufs[i] for i in order]))


def same_outputs(far, near, keys):
    for k in keys:
        a, b = far[k], near[k]
        assert (a is None and b is None) or np.array_equal(np.asarray(a), np.asarray(b)), ("far and near differ in", k)


# ---- the container ----------------------------------------------------------------------------------------------------------------------------
@shapes_wide
def test_compress_and_crc_from_far_resource_offsets(gpu_ctx, oracle, made, fmt, B, base):
    """BlockContainer.compress and .crc (with d_res_crc) with d_in the arena and far d_res_off: packed bytes, tables and checksums are the
    models' and the near container's; the second execution -- a replay -- runs at the moved place, the offsets rewritten in place"""
    import torch
    near, arena = the_store(gpu_ctx, made, fmt, B), FR.arena(gpu_ctx)
    bk, n, nbm, dev = near.bk, near.n, near.nbt, near.dev
    d_off = torch.zeros(n, dtype=torch.int64, device=dev)
    mp, mf, mo, ms = M.model_compress(oracle, near.fmt, near.bufs, B, near.total, near.total)
    bc, rc, kst = K.blocks(near.bufs, B, near.total)
    for place in (FR.PAIR[base][0], FR.MOVED[base][0]):
        with arena.case():
            w, off, _ = FR.plain_window(arena, place, near.bufs, near.total + 3 * n + 64, "resources")
            d_off.copy_(d64(off, dev))
            d_packed = torch.full((near.total + 64,), FILL, dtype=torch.uint8, device=dev)
            d_first, d_boff = torch.full((n + 1,), -1, dtype=torch.int64, device=dev), torch.full((nbm + 1,), -1, dtype=torch.int64, device=dev)
            d_st, d_kst = (torch.full((n,), ST_FILL, dtype=torch.int32, device=dev) for _ in range(2))
            d_bcrc, d_rcrc = (torch.full((k,), CRC_FILL, dtype=torch.int32, device=dev) for k in (nbm, n))
            bk.compress(arena.t, d_off, near.d_len, d_packed, d_first, d_boff, d_st, packed_cap=near.total)
            bk.crc(arena.t, d_off, near.d_len, d_bcrc, d_kst, d_res_crc=d_rcrc)
            gpu_ctx.stream.synchronize()
            first, boff = d_first.cpu().numpy().view(np.uint64), d_boff.cpu().numpy().view(np.uint64)
            assert (first == mf).all() and (boff == mo).all() and [int(x) for x in d_st.cpu().numpy()] == [int(x) for x in ms] == [0] * n
            same_image(d_packed.cpu().numpy(), mp, FILL, "packed bytes")
            assert mp == near.packed and (first == near.first).all() and (boff == near.off).all()
            assert (d_bcrc.cpu().numpy().view(np.uint32) == bc).all() and (d_rcrc.cpu().numpy().view(np.uint32) == rc).all()
            assert (bc[: near.nbt] == near.crc).all() and [int(x) for x in rc] == [zlib.crc32(b) for b in near.bufs]
            assert (d_kst.cpu().numpy() == kst).all()
            assert w.aliases_intact()


def decode(con, bk, d_out, out_off, caps, ranges=None):
    """BlockContainer.decompress of ``con`` into d_out at the absolute offsets ``out_off``: (d_ooff, d_olen, d_st, d_range), synchronised"""
    import torch
    dev = con.dev
    d_ooff, d_ocap = d64(out_off, dev), d64(caps, dev)
    d_olen, d_st = torch.full((con.n,), -1, dtype=torch.int64, device=dev), torch.full((con.n,), ST_FILL, dtype=torch.int32, device=dev)
    d_range = None if ranges is None else d64(np.array(ranges, dtype=np.uint64).reshape(-1), dev)
    bk.decompress(con.d_packed, con.d_first, con.d_boff, con.d_len, d_out, d_ooff, d_ocap, d_olen, d_st, d_range=d_range, packed_len=con.cap)
    con.ctx.stream.synchronize()
    return d_ooff, d_olen, d_st, d_range


@shapes_wide
def test_decompress_and_check_into_far_output_offsets(gpu_ctx, oracle, made, fmt, B, base):
    """BlockContainer.decompress and .check, with and without ranges and with one capacity a byte short, from a far container into far
    d_out_off: statuses, lengths and the whole output window are blocks_model's, check is crc_model's -- healthy, and with a byte of the
    output flipped --, and the near container decodes to the same"""
    import torch
    near, arena = the_store(gpu_ctx, made, fmt, B), FR.arena(gpu_ctx)
    bk, n = near.bk, near.n
    pin, pout = FR.PAIR[base]
    for ranges, short, caps in FR.decode_cases(near.bufs, B):
        ooff, room = near.layout(caps)
        with arena.case():
            far = FR.far_of(oracle, arena, near, pin)
            w = FR.Window(arena, FR.PLACES[pout], room, "output")
            assert pout.startswith("above") or FR.straddles(pout, w.base + ooff[0], caps[0])
            d_ooff, d_olen, d_st, d_range = decode(far, bk, arena.t, [w.base + o for o in ooff], caps, ranges)
            mo, ms = M.model_decompress(oracle, near.fmt, far.packed, far.cap, far.first, far.off, far.lens, B, near.total, caps, ranges)
            st, olen = [int(x) for x in d_st.cpu().numpy()], [int(x) for x in d_olen.cpu().numpy()]
            assert st == ms == [M.BUF if r == short else 0 for r in range(n)]
            assert olen == [len(o) if s == 0 else 0 for o, s in zip(mo, ms)]
            out = w.get()
            same_image(out, [(ooff[r], mo[r]) for r in range(n) if ms[r] == 0], FR.GUARD, "the output window")
            assert w.guards_intact([(0, room)]) and w.aliases_intact()
            near_out = torch.full((room,), FR.GUARD, dtype=torch.uint8, device=near.dev)
            _, n_olen, n_st, _ = decode(near, bk, near_out, ooff, caps, ranges)
            assert torch.equal(n_olen, d_olen) and torch.equal(n_st, d_st) and (near_out.cpu().numpy() == out).all()
            # check: healthy, then with a byte of resource 0's range flipped -- that resource alone fails
            for at in (None, ooff[0] + (B + 5 if ranges is None else 7)):
                d_st2, d_olen2 = d_st.clone(), d_olen.clone()
                if at is not None:
                    arena.t[w.base + at] ^= 0xFF
                bk.check(arena.t, d_ooff, far.d_len, far.d_first, far.d_crc, d_olen2, d_st2, d_range=d_range)
                gpu_ctx.stream.synchronize()
                cs, cl = K.check(w.get(), ooff, near.lens, near.first, near.crc, st, olen, B, near.total, ranges)
                assert ([int(x) for x in d_st2.cpu().numpy()], [int(x) for x in d_olen2.cpu().numpy()]) == (cs, cl)
                assert cs == ([M.DATA if at is not None and short != 0 else st[0]] + st[1:])
            FR.settled(far)


# ---- readers ------------------------------------------------------------------------------------------------------------------------------------
@shapes_wide
def test_reader_from_a_far_container_into_far_output_offsets(gpu_ctx, oracle, made, fmt, B, base):
    """BlockReader.read: the far container through ReadRig.check (model: bytes, lengths, statuses, counts), then the same requests with the
    output offsets far as well: the model's bytes over the guard-filled window, and what the near container gives"""
    import torch
    near, arena = the_store(gpu_ctx, made, fmt, B), FR.arena(gpu_ctx)
    reqs = FR.read_requests(B, near.n)
    caps, bmax = near.wants(reqs), near.budget(reqs)
    ooff, room = near.layout(caps)
    pin, pout = FR.PAIR[base]
    nmo, nms, nmc = near.check(oracle, reqs, crc=True)
    assert nms.count(0) == len(reqs) - 1 and nms[6] != 0
    with arena.case():
        far = FR.far_of(oracle, arena, near, pin)
        mo, ms, mc = far.check(oracle, reqs, crc=True)
        assert (mo, ms, mc) == (nmo, nms, nmc)
        w = FR.Window(arena, FR.PLACES[pout], room, "output")
        assert pout.startswith("above") or FR.straddles(pout, w.base + ooff[0], caps[0])
        rd = near.m.BlockReader(gpu_ctx, near.fmt, B, near.n, near.nbt, len(reqs), bmax)
        d_olen = torch.full((len(reqs),), -1, dtype=torch.int64, device=near.dev)
        d_st = torch.full((len(reqs),), ST_FILL, dtype=torch.int32, device=near.dev)
        for _ in range(2):                                                # (the second execution replays the reader's graph)
            w.refill()
            rd.read(far.d_packed, far.d_first, far.d_boff, far.d_len, d64(np.array(reqs, dtype=np.uint64), near.dev), arena.t,
                    d64([w.base + o for o in ooff], near.dev), d64(caps, near.dev), d_olen, d_st, d_block_crc=far.d_crc, packed_len=far.cap)
            assert rd.counts() == mc
            assert [int(x) for x in d_st.cpu().numpy()] == ms and [int(x) for x in d_olen.cpu().numpy()] == [len(o) if s == 0 else 0 for o, s in zip(mo, ms)]
            same_image(w.get(), [(ooff[q], o) for q, o in enumerate(mo) if ms[q] == 0 and o], FR.GUARD, "the output window")
            assert w.guards_intact([(0, room)]) and w.aliases_intact()
        rd.close()
        FR.settled(far)


# ---- writers ------------------------------------------------------------------------------------------------------------------------------------
@shapes
def test_writer_on_a_far_container_from_far_source_offsets(gpu_ctx, oracle, made, fmt, B, base):
    """BlockWriter.write: the far container through Writes.check (write_model: the whole new container), then with the source bytes in a
    far window as well; both give what the near container gives. One request names no resource."""
    import torch
    near, arena = the_store(gpu_ctx, made, fmt, B), FR.arena(gpu_ctx)
    L = near.lens[0]
    reqs, kinds = FR.write_requests(B, near.n, L)
    srcs = sources(near, reqs, 21, kinds)
    keys = ("image", "off", "crc", "written", "status", "res_status", "counts")
    nmo, ngot = Writes(near).check(oracle, reqs, srcs)
    assert nmo["status"].count(0) == len(reqs) - 1 and nmo["status"][6] != 0 and nmo["res_status"] == [0] * near.n
    pin, pout = FR.PAIR[base]
    with arena.case():
        far = FR.far_of(oracle, arena, near, pin)
        mo, got = Writes(far).check(oracle, reqs, srcs)
        same_outputs(got, ngot, keys)
        wants = near.wants(reqs)
        soff, room = near.layout(wants)
        w = FR.Window(arena, FR.PLACES[pout], room, "sources")
        assert pout.startswith("above") or FR.straddles(pout, w.base + soff[0], wants[0])
        for o, n, s in zip(soff, wants, srcs):
            w.put(o, s[:n])
            w.put_alias(o, bytes(255 - x for x in s[:n]))
        dev, nq = near.dev, len(reqs)
        d_new = torch.full((near.total + 64,), FILL, dtype=torch.uint8, device=dev)
        d_noff = torch.full((near.nbt + 1,), -1, dtype=torch.int64, device=dev)
        d_ncrc = torch.full((near.nbt,), CRC_FILL, dtype=torch.int32, device=dev)
        d_wr, d_st = torch.full((nq,), -1, dtype=torch.int64, device=dev), torch.full((nq,), ST_FILL, dtype=torch.int32, device=dev)
        d_rst = torch.full((near.n,), ST_FILL, dtype=torch.int32, device=dev)
        wr = near.m.BlockWriter(gpu_ctx, near.fmt, B, near.n, near.nbt, nq, near.budget(reqs))
        wr.write(far.d_packed, far.d_first, far.d_boff, far.d_len, d64(np.array(reqs, dtype=np.uint64), dev), arena.t, d64([w.base + o for o in soff], dev),
                 d_new, d_noff, d_wr, d_st, d_rst, d_block_crc=far.d_crc, d_new_block_crc=d_ncrc, packed_len=far.cap, new_cap=near.total)
        counts = wr.counts()
        wr.close()
        mine = {"image": d_new.cpu().numpy(), "off": d_noff.cpu().numpy().view(np.uint64), "crc": d_ncrc.cpu().numpy().view(np.uint32),
                "written": [int(x) for x in d_wr.cpu().numpy().view(np.uint64)], "status": [int(x) for x in d_st.cpu().numpy()],
                "res_status": [int(x) for x in d_rst.cpu().numpy()], "counts": counts}
        same_outputs(mine, ngot, keys)
        assert w.guards_intact([(o, n) for o, n in zip(soff, wants)]) and w.aliases_intact()
        FR.settled(far)


@shapes
def test_resize_of_a_far_container(gpu_ctx, oracle, made, fmt, B, base):
    """BlockWriter.resize, truncate and zero-extend in one call: resize_model's new container, read back, and the near container's"""
    near, arena = the_store(gpu_ctx, made, fmt, B), FR.arena(gpu_ctx)
    want = FR.resize_want(near.lens, B)
    keys = ("image", "first", "off", "crc", "new_len", "status", "counts")
    zs = Resizes(near)
    nmo, ngot = zs.check(oracle, want)
    assert nmo["res_status"] == [0] * near.n and nmo["new_len"] == want
    with arena.case():
        far = FR.far_of(oracle, arena, near, FR.PAIR[base][0])
        fz = Resizes(far)
        mo, got = fz.check(oracle, want)
        same_outputs(got, ngot, keys)
        mo, got = fz.check(oracle, want, new_cap=int(nmo["off"][1]) + 1)      # new_cap inside the second block: refusals
        assert M.BUF in mo["res_status"]
        fz.big.close()
        FR.settled(far)
    zs.big.close()


# ---- splicers -----------------------------------------------------------------------------------------------------------------------------------
def splices_over(near0, near1):
    """blocks_rig.Extents (and with it Splices) over two containers that exist already"""
    zs = Extents.__new__(Extents)
    zs.rig = zs.src = [near0, near1]
    zs.m, zs.ctx, zs.fmt, zs.B, zs.dev = near0.m, near0.ctx, near0.fmt, near0.B, near0.dev
    zs.room = 2 * max(r.total for r in zs.rig) + 3 * zs.B
    return zs


def two_far(oracle, arena, made, gpu_ctx, fmt, B, base):
    """(the store, the same buffers in another order as a second container, their far copies at the two places of the base)"""
    n0, n1 = the_store(gpu_ctx, made, fmt, B), the_store(gpu_ctx, made, fmt, B, FR.SECOND, "second")
    return n0, n1, FR.far_of(oracle, arena, n0, FR.PAIR[base][0]), FR.far_of(oracle, arena, n1, FR.PAIR[base][1])


@shapes
def test_splices_of_two_far_sources(gpu_ctx, oracle, made, fmt, B, base):
    """BlockSplicer.splice and .splice_extents over two far sources at different places (the move kernel's row-address column): the
    models' new container, and the one the near sources give. One pick and one extent list are refused."""
    arena = FR.arena(gpu_ctx)
    keys = ("image", "first", "off", "crc", "new_len", "status")
    with arena.case():
        n0, n1, f0, f1 = two_far(oracle, arena, made, gpu_ctx, fmt, B, base)
        zs = splices_over(n0, n1)
        picks = FR.PICKS
        nbt = n0.nbt + n1.nbt
        nmo, ngot = Splices.check(zs, picks, nbt)
        assert nmo["status"] == [0, 0, 0, 0, M.ARG, 0, 0]
        mo, got = Splices.check(zs, picks, nbt, srcs=[f0, f1])
        same_outputs(got, ngot, keys)
        resources = FR.EXTENTS
        nmo, ngot = zs.check(resources, nbt)
        assert nmo["status"] == [0, 0, 0, M.ARG, 0, 0] and nmo["new_len"][2] == 17
        mo, got = zs.check(resources, nbt, srcs=[f0, f1])
        same_outputs(got, ngot, keys)
        FR.settled(f0, f1)


# ---- dedupers -----------------------------------------------------------------------------------------------------------------------------------
LISTS = ("delta_first", "delta_ext", "patch_first", "patch_ext", "count", "status")


@shapes
def test_dedup_of_two_far_sources(gpu_ctx, oracle, made, fmt, B, base):
    """BlockDeduper.dedup over two far sources, with and without checksums; then dedup_model's full-key collision (equal lengths, CRC
    words and row ends), where only the confirm pass -- which reads the far stored bytes -- tells the twin apart"""
    arena = FR.arena(gpu_ctx)
    with arena.case():
        n0, n1, f0, f1 = two_far(oracle, arena, made, gpu_ctx, fmt, B, base)
        zs = splices_over(n0, n1)
        for with_crc in (True, False):
            nmo, _ = check_dedup(zs, [n0, n1], with_crc)
            mo, _ = check_dedup(zs, [f0, f1], with_crc)
            assert FR.same(mo, nmo) and mo["rep"] == [0, 1, 2, 2, 0, 1] and mo["status"] == [0] * 6
        FR.settled(f0, f1)
    bufs0, bufs1 = FR.collision_buffers(B)
    c0 = made((fmt, B, "collision0"), lambda: Container.make(gpu_ctx, FMTS[fmt], B, bufs0))
    c1 = made((fmt, B, "collision1"), lambda: Container.make(gpu_ctx, FMTS[fmt], B, bufs1))
    assert c0.packed[: len(bufs0[0])] == bufs0[0] and (c0.crc[:4] == c1.crc[:4]).all()
    with arena.case():
        f0, f1 = FR.far_of(oracle, arena, c0, FR.PAIR[base][0]), FR.far_of(oracle, arena, c1, FR.PAIR[base][1])
        mo, _ = check_dedup(splices_over(c0, c1), [f0, f1], True)
        assert mo["rep"] == [0, 1, 2, 0] and mo["count"][0] == 3 and mo["count"][3] == 1
        FR.settled(f0, f1)


def edited_store(ctx, made, fmt, B):
    return made((fmt, B, "edited"), lambda: Container.make(ctx, FMTS[fmt], B, FR.edited_buffers(B)))


@shapes
def test_match_and_diff_of_two_far_sources(gpu_ctx, oracle, made, fmt, B, base):
    """BlockDeduper.match and .diff of a far store and a far later version of it, then delta and patch spliced from the calls' own lists
    over the far views: match_model's and diff_model's lists and containers, and those of the near pair"""
    arena = FR.arena(gpu_ctx)
    n0, n1 = the_store(gpu_ctx, made, fmt, B), edited_store(gpu_ctx, made, fmt, B)
    nmo, nouts = check_match([n0], n1)
    nmd, nmb = match_rebuild([n0], n1, nmo, nouts)
    pairs = F.default_pairs(n0.model(), n1.model())
    dmo, douts = check_diff(n0, n1, pairs)
    dmd, dmb = diff_rebuild(n0, n1, pairs, dmo, douts)
    assert nmo["count"][2] > 0 and dmo["count"][0] > 0                    # something changed, something is carried
    with arena.case():
        f0, f1 = FR.far_of(oracle, arena, n0, FR.PAIR[base][0]), FR.far_of(oracle, arena, n1, FR.PAIR[base][1])
        mo, outs = check_match([f0], f1)
        assert all(FR.same(mo[k], nmo[k], k) for k in LISTS + ("cls",))
        md, mb = match_rebuild([f0], f1, mo, outs, same=False)
        for far, near in ((md, nmd), (mb, nmb)):
            same_outputs(far, near, ("packed", "first", "off", "crc", "new_len", "status"))
        assert F.default_pairs(f0.model(), f1.model()) == pairs
        mo, outs = check_diff(f0, f1, pairs)
        assert all(FR.same(mo[k], dmo[k], k) for k in LISTS + ("changed",))
        md, mb = diff_rebuild(f0, f1, pairs, mo, outs, same=False)
        for far, near in ((md, dmd), (mb, dmb)):
            same_outputs(far, near, ("packed", "first", "off", "crc", "new_len", "status"))
        FR.settled(f0, f1)


# ---- digester and syncers ------------------------------------------------------------------------------------------------------------------------
class FarDRig(DRig):
    """test_gpu_digest's rig (a syncer and a digest syncer over one set of guarded outputs) with its raw units in a far window"""

    def place(self, arena, place):
        self.arena, self.where, self.d_in = arena, place, arena.t

    def load(self, units):
        self.units = [bytes(u) for u in units]
        self.win, self.offs, self.rel = FR.plain_window(self.arena, self.where, self.units, sum(len(u) for u in units) + 3 * self.nu + 64, "units")
        self.d_off.copy_(d64(self.offs, self.dev, self.nu)); self.d_len.copy_(d64([len(u) for u in units], self.dev, self.nu))
        self.outs.reset(); self.res_status.fill_(SENT32)

    def rebuild(self, store, mo):
        """the consequence on the device, as test_gpu_sync.py rebuilds it, into a buffer as long as the window: the literal runs copied,
        the hits read by a BlockReader at the call's own d_req_off less the window's base"""
        import torch
        base = self.win.base
        out = torch.full((self.win.room,), FILL, dtype=torch.uint8, device=self.dev)
        lit = self.outs["lit"].cpu().numpy().view(np.uint64)
        for i in range(mo["count"][5]):
            o, ln = int(lit[2 * i]), int(lit[2 * i + 1])
            out[o - base: o - base + ln] = self.d_in[o: o + ln]
        hits = mo["count"][4]
        d_roff = self.outs["req_off"].clone()
        d_roff[:hits] -= base
        rd = self.m.BlockReader(self.ctx, self.fmt, self.B, store.n, store.nbt, self.nc, self.nc)
        d_len, d_st = torch.zeros(self.nc, dtype=torch.int64, device=self.dev), torch.zeros(self.nc, dtype=torch.int32, device=self.dev)
        rd.read(store.d_packed, store.d_first, store.d_boff, store.d_len, self.outs["req"], out, d_roff, d64([self.B] * self.nc, self.dev), d_len, d_st,
                d_block_crc=store.d_crc, packed_len=store.plen)
        self.ctx.stream.synchronize()
        rd.close()
        assert [int(x) for x in d_st.cpu().numpy()] == [0] * hits + [M.ARG] * (self.nc - hits)
        same_image(out.cpu().numpy(), [(self.rel[u], self.units[u]) for u in range(self.nu) if mo["status"][u] == 0], FILL, "the rebuilt batch")


@shapes
@pytest.mark.parametrize("case", ["edits", "seams"])
def test_sync_and_sync_digest_of_a_far_store_and_far_units(gpu_ctx, oracle, made, fmt, B, base, case):
    """BlockSyncer.sync and .sync_digest: a far store, the raw units of sync_model.cases at far unit offsets. Both against their models
    and against each other (DRig.check), the hits and runs as for the near store and near units but for the unit offsets, and the batch
    rebuilt on the device from the call's own lists"""
    near, arena = the_store(gpu_ctx, made, fmt, B), FR.arena(gpu_ctx)
    digs = made((fmt, B, "digests"), lambda: digests_of(near))
    units = Y.cases(B)[case]
    room = sum(len(u) for u in units)
    nc = 2 * (room // B) + 8
    nrig = DRig(near, len(units), room, nc)
    nmo, _ = nrig.check(near, digs[0], digs[1], units)
    nrig.close()
    pin, pout = FR.PAIR[base]
    with arena.case():
        far = FR.far_of(oracle, arena, near, pin)
        rig = FarDRig(far, len(units), room, nc)
        rig.place(arena, pout)
        mo, _ = rig.check(far, digs[0], digs[1], units)
        assert all(FR.same(mo[k], nmo[k], k) for k in ("res_status", "status", "hit_first", "req", "lit_first", "count", "hits", "literals", "kept"))
        assert sum(len(h) for h in mo["hits"]) > 0 and mo["req_off"] == [x - nrig.offs[0] + rig.offs[0] for x in nmo["req_off"]]
        plain = Y.model_sync(oracle, far.fmt, far.model(), rig.units, rig.offs, B, rig.in_total_max, nc)
        assert plain["req"] == mo["req"] and plain["req_off"] == mo["req_off"] and plain["lit"] == mo["lit"]
        rig.rebuild(far, mo)
        assert rig.win.aliases_intact() and bytes(rig.win.get()) == bytes(odd_offsets(rig.units, rig.win.room)[1])
        rig.close()
        FR.settled(far)


@shapes
def test_digester_blocks_and_check_at_far_offsets(gpu_ctx, oracle, made, fmt, B, base):
    """BlockDigester.blocks over far d_res_off, and .check behind a decompress into far d_out_off -- healthy, and with a byte flipped:
    digest_model's column and verdicts"""
    import torch
    near, arena = the_store(gpu_ctx, made, fmt, B), FR.arena(gpu_ctx)
    n, dev = near.n, near.dev
    dg = near.m.BlockDigester(gpu_ctx, B, n, near.total)
    want, wst = G.model_digests(near.bufs, B, near.total)
    pin, pout = FR.PAIR[base]
    with arena.case():
        w, off, _ = FR.plain_window(arena, pin, near.bufs, near.total + 3 * n + 64, "resources")
        d_dig = torch.full((4 * dg.n_blocks_max + 4,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        d_st = torch.full((n,), ST_FILL, dtype=torch.int32, device=dev)
        dg.blocks(arena.t, d64(off, dev), near.d_len, d_dig, d_st)
        gpu_ctx.stream.synchronize()
        got = d_dig.cpu().numpy().view(np.uint32)
        assert (got[: 4 * dg.n_blocks_max].reshape(-1, 4) == want).all() and (got[4 * dg.n_blocks_max:] == 0x5A5A5A5A).all()
        assert [int(x) for x in d_st.cpu().numpy()] == [int(x) for x in wst] == [0] * n and w.aliases_intact()
    ranges, _, caps = FR.decode_cases(near.bufs, B)[1]
    ooff, room = near.layout(caps)
    with arena.case():
        far = FR.far_of(oracle, arena, near, pin)
        w = FR.Window(arena, FR.PLACES[pout], room, "output")
        d_ooff, d_olen, d_st, d_range = decode(far, near.bk, arena.t, [w.base + o for o in ooff], caps, ranges)
        st, olen = [int(x) for x in d_st.cpu().numpy()], [int(x) for x in d_olen.cpu().numpy()]
        assert st == [0] * n
        for at in (None, ooff[0] + B + 5):
            if at is not None:
                arena.t[w.base + at] ^= 0xFF
            d_st2, d_olen2 = d_st.clone(), d_olen.clone()
            dg.check(arena.t, d_ooff, far.d_len, far.d_first, d_dig, d_olen2, d_st2, d_range=d_range)
            gpu_ctx.stream.synchronize()
            ms, ml = G.model_check(w.get(), ooff, near.lens, near.first, got, st, olen, B, near.total, ranges)
            assert ([int(x) for x in d_st2.cpu().numpy()], [int(x) for x in d_olen2.cpu().numpy()]) == (ms, ml)
            assert ms == ([0, 0, 0] if at is None else [M.DATA, 0, 0])
        FR.settled(far)
    dg.close()


# ---- the transcoder ---------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("base", list(FR.BASES))
@pytest.mark.parametrize("name,f1,B1,f2,B2", FR.TRANSCODES)
def test_transcode_of_a_far_source(gpu_ctx, oracle, name, f1, B1, f2, B2, base):
    """BlockTranscoder.transcode: an LZNT1 join 4096 -> 16384 and a split 16384 -> 4096 (the carry paths, whose row addresses point into
    the far source), a codec change LZNT1 -> Xpress, and the 64 KiB Xpress+Huffman store to Xpress: transcode_model's container and
    counts, and what the near source gives"""
    arena = FR.arena(gpu_ctx)
    src = Source(oracle, f1, B1, Y.store_buffers(min(B1, B2) if name != "wide" else B1))
    run = Run(gpu_ctx, src, f2, B2)
    ngot = run.go()
    same_transcode(ngot, run.model(oracle))
    at = FR.PLACES[FR.PAIR[base][0]]
    with arena.case():
        w = FR.Window(arena, at, len(src.packed), "source")
        w.put(0, src.packed)
        other = Source(oracle, f1, B1, [bytes(255 - x for x in b) for b in src.bufs])
        w.put_alias(0, (other.packed + bytes(len(src.packed)))[: len(src.packed)])
        far_src = copy.copy(src)
        far_src.off = src.off + np.uint64(at)
        run.src, run.packed = far_src, FR.FarBytes(at, src.packed)
        run.d_packed, run.d_off = arena.t, d64(far_src.off, run.dev)
        got = run.go()
        want = run.model(oracle)
        same_transcode(got, want)
        same_outputs(got, ngot, ("image", "first", "off", "crc", "status", "counts"))
        assert got["status"][: run.n] == [0] * run.n and (name not in ("join", "split") or want[5][2] > 0 or want[5][1] > 0)
        assert bytes(w.get()) == src.packed and w.guards_intact([(0, w.room)]) and w.aliases_intact()
    run.close()


# ---- parity, salvage and repair ---------------------------------------------------------------------------------------------------------------
@shapes
def test_parity_build_and_rebuild_of_a_far_container(gpu_ctx, oracle, made, fmt, B, base):
    """BlockParity.build over the far store, and .rebuild of a far copy that lost two rows: parity_model's rows and fixes, and those the
    near containers give"""
    near, arena = the_store(gpu_ctx, made, fmt, B), FR.arena(gpu_ctx)
    nb = int(near.first[-1])
    pr = near.m.BlockParity(gpu_ctx, B, near.nbt, *FR.PARITY)
    nmo, nset = check_build(pr, near)
    par_len = int(nmo["par_off"][-1])
    lost = [0, nb - 1]                                                    # the first stored block (it straddles) and the last one
    dam, ver = lose(near, lost)
    dam.decoy = near.packed                                               # where a cut offset reads, nothing is lost
    nfix, _ = check_rebuild(pr, dam, ver, nset, par_len)
    assert nmo["status"] == 0 and nfix["status"] == 0 and nfix["count"][0] >= 2
    with arena.case():
        far = FR.far_of(oracle, arena, near, FR.PAIR[base][0])
        mo, pset = check_build(pr, far)
        assert all(np.array_equal(mo[k], nmo[k]) for k in ("par_off", "par_crc", "row_len", "head", "status")) and mo["pieces"] == nmo["pieces"]
        FR.settled(far)
    with arena.case():
        fdam = FR.far_of(oracle, arena, dam, FR.PAIR[base][0])
        fix, _ = check_rebuild(pr, fdam, ver, pset, par_len, outs=FixOuts(near.dev, near.nbt, near.plen + 64))
        assert all(np.array_equal(fix[k], nfix[k]) for k in ("fix_off", "fix_verdict", "count", "status")) and fix["pieces"] == nfix["pieces"]
        FR.settled(fdam)
    pr.close()


@shapes
def test_salvage_and_repair_of_a_far_primary_and_a_far_mirror(gpu_ctx, oracle, made, fmt, B, base):
    """BlockContainer.salvage of a damaged far primary and of its healthy far mirror (masked by the primary's verdicts), then
    BlockDeduper.repair over the two and the splice of its lists: repair_model's verdicts, lists and container -- the undamaged one,
    byte for byte -- and what the near pair gives. The salvage writes into far output offsets as well."""
    import torch
    near, arena = the_store(gpu_ctx, made, fmt, B), FR.arena(gpu_ctx)
    dam = near.edited(packed=FR.damaged_stored(oracle, near))             # a raw block hurt (seen by its checksum), a compressed one undecodable
    dam.decoy = near.packed
    nmo, _, _ = check_salvage(oracle, near, dam)
    nmi, _, _ = check_salvage(oracle, near, near, only=nmo["verdict"])
    nro, nouts = check_repair([dam, near], [nmo["verdict"], nmi["verdict"]])
    assert nmo["bad"][0] == 2 and nro["status"] == [0] * near.n and nro["count"][1] == 0
    pin, pout = FR.PAIR[base]
    with arena.case():
        fdam, fmir = FR.far_of(oracle, arena, dam, pin), FR.far_of(oracle, arena, near, pout)
        mo, outs, out_off = check_salvage(oracle, near, fdam)
        mi, _, _ = check_salvage(oracle, near, fmir, only=mo["verdict"])
        for far, nr in ((mo, nmo), (mi, nmi)):
            same_outputs(far, nr, ("verdict", "bad", "out_len", "status", "count"))
        ro, routs = check_repair([fdam, fmir], [mo["verdict"], mi["verdict"]])
        assert all(FR.same(ro[k], nro[k], k) for k in ("ext_first", "ext", "fixed", "lost", "status", "count"))
        built = Spliced(near.dev, near.n, near.nbt, 2 * near.plen + 32, True)
        repair_rebuild([fdam, fmir], ro, routs, healthy=near, built=built)
        FR.settled(fdam, fmir)
    with arena.case():                                                    # salvage once more, its output offsets far as well
        fdam = FR.far_of(oracle, arena, dam, pin)
        caps = list(near.lens)
        ooff, room = near.layout(caps)
        w = FR.Window(arena, FR.PLACES[pout], room, "output")
        dev = near.dev
        full = lambda k, v, t: torch.full((k,), v, dtype=t, device=dev)
        d_olen, d_count = full(near.n, -1, torch.int64), full(4, -1, torch.int64)
        d_bad, d_ver, d_st = full(near.n, ST_FILL, torch.int32), full(near.nbt, ST_FILL, torch.int32), full(near.n, ST_FILL, torch.int32)
        near.bk.salvage(fdam.d_packed, fdam.d_first, fdam.d_boff, fdam.d_len, arena.t, d64([w.base + o for o in ooff], dev), d64(caps, dev), d_olen, d_bad,
                        d_ver, d_count, d_st, d_block_crc=fdam.d_crc, packed_len=fdam.cap)
        gpu_ctx.stream.synchronize()
        import repair_model as P
        assert [int(x) for x in d_ver.cpu().numpy()] == [int(x) for x in nmo["verdict"]] and [int(x) for x in d_st.cpu().numpy()] == nmo["status"]
        assert [int(x) for x in d_olen.cpu().numpy()] == [int(x) for x in nmo["out_len"]]
        assert [int(x) for x in d_bad.cpu().numpy()] == nmo["bad"] and [int(x) for x in d_count.cpu().numpy()] == nmo["count"]
        same_image(w.get(), P.image_pieces(nmo, ooff, B), FR.GUARD, "the salvaged output window")
        assert w.guards_intact([(0, room)]) and w.aliases_intact()
        FR.settled(fdam)
