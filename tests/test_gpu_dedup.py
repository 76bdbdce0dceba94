"""GPU: mscomp_amd_deduper_dedup against the model of tests/dedup_model.py -- every entry of the five outputs compared with sentinel-filled
arrays that are longer than the call may write (so a write behind N, or behind 2 n_res_total in d_pick, fails) -- on the containers of
tests/blocks_rig.Container; then the picks spliced on the GPU by a splicer made for n_res_total picks, held to the header's consequence and,
where the sources are healthy, byte for byte to BlockContainer.compress + .crc of the unique data."""
import numpy as np
import pytest

import blocks_model as M
import dedup_model as D
import read_model as R
import splice_model as S
from blocks_rig import Container, Splices, check_dedup, dedup_outs, dedup_views, memo, DEDUP_EXACT, FMTS, BLOCKS, MIXED, SENT
from dedup_model import EMPTY, expect_two_orders
from splice_model import ORDER2

pytestmark = pytest.mark.gpu
M64 = M.M64


def splice_picks(zs, srcs, mo, outs, with_crc=True, healthy=None):
    """d_pick as the call left it, padding and all, through a splicer made for n_res_total picks: the result against the splice model and
    the consequence; healthy = the sources' buffers, when the result must also be what compress + crc write for the unique ones"""
    npk, models = outs.n_max, [s.model() for s in srcs]
    picks = [(mo["pick"][2 * p], mo["pick"][2 * p + 1]) for p in range(npk)]
    total = sum(int(models[s][4][r]) for s, r in picks[: mo["count"][0]])     # the unique resources' data bytes
    nbt = npk + total // zs.B if healthy else sum(s.nbt for s in srcs)          # (healthy: the table BlockContainer makes for that data)
    so = zs.outputs(npk, nbt)
    d_new, d_first, d_off, d_crc, d_len, d_st = so.tensors()
    sp = zs.m.BlockSplicer(zs.ctx, zs.B, len(srcs), npk, nbt)
    sp.splice(dedup_views(srcs, with_crc), outs["pick"], d_new, d_first, d_off, d_len, d_st, d_new_block_crc=d_crc if with_crc else None, new_cap=zs.room)
    got = zs.pull(so)
    sp.close()
    ms = S.model_splice(models, picks, zs.B, nbt, zs.room, with_crc=with_crc)
    zs.compare(got, ms, npk, nbt, with_crc)
    D.holds_consequence(models, zs.B, with_crc, mo, {"packed": got["image"], "first": got["first"], "off": got["off"], "crc": got["crc"], "new_len": got["new_len"]})
    if healthy and with_crc:
        data = [healthy[s][r] for s, r in picks[: mo["count"][0]]] + [b""] * (npk - mo["count"][0])
        zs.check_consequence(got, data, nbt)
    return got


@pytest.fixture(scope="module")
def rigs(gpu_ctx):
    yield from memo(lambda fmt, B: Splices(gpu_ctx, FMTS[fmt], B))


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_two_containers_in_two_orders(rigs, fmt, B):
    zs = rigs(fmt, B)
    n = zs.rig[0].n
    for with_crc in (True, False):
        mo, outs = check_dedup(zs, zs.src, with_crc)
        assert mo["status"] == [0] * (2 * n) and mo["rep"] == expect_two_orders(n) and mo["count"][0] == n - 1 and mo["count"][3] == 0
        assert mo["count"][2] == zs.rig[1].plen                     # everything the second container stores is saved (the second empty stores nothing)
        splice_picks(zs, zs.src, mo, outs, with_crc, healthy=[r.bufs for r in zs.rig])


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_one_container_alone(rigs, fmt, B):
    zs = rigs(fmt, B)
    n = zs.rig[0].n
    mo, outs = check_dedup(zs, zs.src[:1])
    assert mo["rep"] == list(range(n - 1)) + [EMPTY] and mo["count"] == [n - 1, n, 0, 0]
    splice_picks(zs, zs.src[:1], mo, outs, healthy=[zs.rig[0].bufs])


def stored_raw(rig):
    """every block of the rig's container is stored raw: the stored bytes are the data"""
    return rig.packed == b"".join(rig.bufs)


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_full_key_collision_with_checksums(gpu_ctx, fmt, B):
    """equal lengths, CRC words and row ends: only the confirm pass can tell the twin apart; the resource behind it is a true duplicate"""
    base = M.build({"kind": "random", "seed": 9, "mult": 3, "add": 17}, B)
    twin = D.crc_twin(base, B + B // 2)
    zs = Splices(gpu_ctx, FMTS[fmt], B, bufs0=[base, np.random.RandomState(3).bytes(7)], bufs1=[twin, base])
    assert twin != base and stored_raw(zs.rig[0]) and stored_raw(zs.rig[1])
    assert (zs.rig[0].crc[:4] == zs.rig[1].crc[:4]).all()          # the case is not vacuous: one key tuple, checksums and all
    mo, outs = check_dedup(zs, zs.src, True)
    assert mo["rep"] == [0, 1, 2, 0] and mo["count"][0] == 3 and mo["count"][3] == 1
    splice_picks(zs, zs.src, mo, outs, healthy=[r.bufs for r in zs.rig])
    zs.close()


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_several_classes_under_one_key(gpu_ctx, fmt, B):
    """A B C A B C, one length, equal row ends, no checksums: the settle stage makes B and C representatives and finds their copies"""
    a, b, c = D.same_ends([M.build({"kind": "random", "seed": 40 + k, "mult": 2, "add": 100}, B) for k in range(3)], B)
    zs = Splices(gpu_ctx, FMTS[fmt], B, bufs0=[a, b, c], bufs1=[a, b, c])
    assert len({a, b, c}) == 3 and stored_raw(zs.rig[0])
    mo, outs = check_dedup(zs, zs.src, False)
    assert mo["rep"] == [0, 1, 2, 0, 1, 2] and mo["count"] == [3, 6, 3 * len(a), 4]
    splice_picks(zs, zs.src, mo, outs, False)
    mo, outs = check_dedup(zs, zs.src, True)                       # with checksums every class has its own key
    assert mo["rep"] == [0, 1, 2, 0, 1, 2] and mo["count"][3] == 0
    zs.close()


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_refusals(rigs, fmt, B):
    zs = rigs(fmt, B)
    rig = zs.rig[0]
    n, lens = rig.n, rig.lens
    twin = lambda r: n + ORDER2.index(r)                           # where the second container holds resource r of the first
    falling = rig.first.copy(); falling[3] = falling[4] + np.uint64(1)     # resource 3 by rule 1; resource 2 gets a row too many: rule 2
    beyond = rig.first.copy(); beyond[n] = np.uint64(rig.nbt + 1)          # the last, empty resource by rule 1
    odd = list(lens); odd[MIXED] += B                                      # rule 2
    j = int(rig.first[MIXED])
    past = rig.off.copy(); past[j + 2:] = np.uint64(rig.plen + 1)          # rule 3: row 1 of MIXED ends beyond packed_len, and so does every row behind it
    back = rig.off.copy(); back[j + 2] = back[j + 1] - np.uint64(1)        # rule 3: a decreasing entry inside MIXED
    for hurt, bad in ((rig.edited(first=falling), {3: M.ARG, 2: M.DATA}), (rig.edited(first=beyond), {n - 1: M.ARG}), (rig.edited(lens=odd), {MIXED: M.DATA}),
                      (rig.edited(off=past), {r: M.DATA for r in range(MIXED, n) if lens[r]}), (rig.edited(off=back), {MIXED: M.DATA})):
        srcs = [hurt, zs.src[1]]
        mo, outs = check_dedup(zs, srcs)
        assert mo["status"] == [bad.get(r, 0) for r in range(n)] + [0] * n
        for r in bad:                                              # its own representative, and its healthy twin does not point at it
            assert mo["rep"][r] == r and mo["rep"][twin(r)] != r
        for r in range(n):
            if r not in bad and lens[r]:
                assert mo["rep"][twin(r)] == r
        splice_picks(zs, srcs, mo, outs)


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_alignment(gpu_ctx, fmt, B):
    """one resource of raw and compressed rows alone in a container, and fifteen copies of it in another behind resources of 1 .. 16 bytes
    that put them at every other residue mod 16; then single stored bytes of a compressed row flipped"""
    x = R.buffers(B)[MIXED]
    alone = Container.make(gpu_ctx, FMTS[fmt], B, [x])
    size, rs, bufs, at = alone.plen, np.random.RandomState(5), [], 0
    for k in range(1, 16):
        pad = (k - at) % 16 or 16
        bufs += [rs.bytes(pad), x]
        at += pad + size
    zs = Splices(gpu_ctx, FMTS[fmt], B, bufs0=[x], bufs1=bufs)
    alone.close()
    one, many = zs.rig
    starts = [int(many.off[int(many.first[2 * k + 1])]) for k in range(15)]
    assert one.plen == size and [s % 16 for s in starts] == list(range(1, 16))
    mo, outs = check_dedup(zs, zs.src)
    assert [mo["rep"][2 + 2 * k] for k in range(15)] == [0] * 15 and mo["count"][3] == 0
    # row 1 of the resource is text: stored compressed, the same length on both sides whatever byte of it is flipped
    o0, o1 = int(one.off[1]), int(one.off[2])
    assert 16 < o1 - o0 < B

    def flipped(rig, base, where):
        hurt = bytearray(rig.packed); hurt[base + where] ^= 0x40
        return rig.edited(packed=bytes(hurt))
    for where, refuted in ((o0, 0), (o1 - 1, 0), ((o0 + o1) // 2, 15)):      # a first or last byte changes the key; a middle one only the bytes
        mo, outs = check_dedup(zs, [flipped(one, 0, where), zs.src[1]])
        assert [mo["rep"][2 + 2 * k] for k in range(15)] == [2] * 15 and mo["count"][3] == refuted
        mo, outs = check_dedup(zs, [zs.src[0], flipped(many, starts[6], where)])
        assert [mo["rep"][2 + 2 * k] for k in range(15)] == [0] * 6 + [14] + [0] * 8 and mo["count"][3] == (1 if refuted else 0)
    zs.close()


def test_bounds(rigs):
    import torch
    zs = rigs("xpress", 4096)
    m, B, n = zs.m, zs.B, zs.rig[0].n
    rows = sum(s.nbt for s in zs.src)
    # room for more resources than there are: the padding of d_pick reaches 2 n_res_total, the other arrays end at N
    mo, outs = check_dedup(zs, zs.src, n_max=2 * n + 5, rows_max=rows + 9)
    assert mo["pick"][2 * (n - 1):] == [M64] * (2 * (n + 6))
    splice_picks(zs, zs.src, mo, outs, healthy=[r.bufs for r in zs.rig])
    # no resources at all
    none = [r.edited(lens=[], nbt=0) for r in zs.rig]
    mo, outs = check_dedup(zs, none, n_max=3, rows_max=0)
    assert mo["count"] == [0, 0, 0, 0] and mo["pick"] == [M64] * 6
    mo, outs = check_dedup(zs, none, n_max=0, rows_max=0)
    assert mo["count"] == [0, 0, 0, 0] and mo["pick"] == []
    dd = m.BlockDeduper(zs.ctx, B, 2, 0, 0)
    cnt = torch.full((4,), SENT, dtype=torch.int64, device=zs.dev)
    dd.dedup(dedup_views(none, True), None, None, None, cnt, None)       # N = 0: d_count alone is required
    zs.ctx.stream.synchronize()
    assert cnt.cpu().tolist() == [0, 0, 0, 0]
    dd.close()
    # refused on the host, nothing launched: too many resources, too many rows, each output missing in turn, a view without a table
    outs = dedup_outs(zs.dev, 2 * n)
    full = outs.tensors()
    missing = [full[:k] + (None,) + full[k + 1:] for k in range(5)]
    for n_max, rows_max, srcs, args in ((2 * n - 1, rows, dedup_views(zs.src, True), full), (2 * n, rows - 1, dedup_views(zs.src, True), full),
                                        *[(2 * n, rows, dedup_views(zs.src, True), a) for a in missing],
                                        (2 * n, rows, [zs.src[0].view(), zs.src[1].view()[:1] + (None,) + zs.src[1].view()[2:]], outs.tensors())):
        dd = m.BlockDeduper(zs.ctx, B, 2, n_max, rows_max)
        with pytest.raises(m.MSCompError) as e:
            dd.dedup(srcs, *args)
        assert e.value.status == m.MSCOMP_ARG_ERROR
        dd.close()
    dd = m.BlockDeduper(zs.ctx, B, 2, 2 * n, rows)                 # no sources at all (the binding always passes some: the export itself)
    assert zs.ctx.lib.mscomp_amd_deduper_dedup(dd._h, None, *[t.data_ptr() for t in full]) == m.MSCOMP_ARG_ERROR
    dd.close()
    torch.cuda.synchronize()
    assert outs.untouched()


@pytest.mark.parametrize("B", BLOCKS)
def test_a_row_longer_than_a_block(gpu_ctx, B):
    """nothing bounds a stored length but packed_len: a table edited so that a resource of B bytes has ONE row of 5 B stored bytes passes
    rules 1-3, and two such resources that differ in one byte behind 4 B -- behind the row's last 16 KiB piece at either block size, far
    from the row's ends, under equal CRC words -- are told apart by the confirm pass alone; two that do not differ are equal"""
    data = M.build({"kind": "random", "seed": 31, "mult": 5, "add": 0}, B)
    other = bytearray(data); other[4 * B + 100] ^= 0x10
    zs = Splices(gpu_ctx, FMTS["xpress"], B, bufs0=[data], bufs1=[bytes(other)])
    assert stored_raw(zs.rig[0]) and stored_raw(zs.rig[1]) and 4 * B + 100 >= max(B, 16384)

    def one_row(rig):
        return rig.edited(first=np.array([0, 1], dtype=np.uint64), off=np.array([0] + [5 * B] * rig.nbt, dtype=np.uint64), lens=[B])
    for srcs, rep, refuted in (([one_row(zs.rig[0]), one_row(zs.rig[1])], [0, 1], 1), ([one_row(zs.rig[0]), one_row(zs.rig[0])], [0, 0], 0)):
        for with_crc in (True, False):
            mo, outs = check_dedup(zs, srcs, with_crc)
            assert mo["status"] == [0, 0] and mo["rep"] == rep and mo["count"][3] == refuted
            splice_picks(zs, srcs, mo, outs, with_crc)
    zs.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_three_executions_are_identical(rigs, fmt):
    """one deduper, the same arguments three times, a full key collision among the sources so that the flags, the settle stage and the early
    exit all take part: the same outputs every time, counts included. (The library replays the call's own graph from the second execution
    on; no export says whether an execution was a replay, so that is not asserted here.)"""
    B = 4096
    zs = rigs(fmt, B)
    one = zs.rig[0]
    j = int(one.first[MIXED])
    where = (int(one.off[j + 1]) + int(one.off[j + 2])) // 2       # a middle byte of MIXED's compressed row: same key, other bytes
    hurt = bytearray(one.packed); hurt[where] ^= 0x01
    srcs = [one.edited(packed=bytes(hurt)), zs.src[1]]
    N, rows = 2 * one.n, sum(s.nbt for s in srcs)
    dd = zs.m.BlockDeduper(zs.ctx, B, 2, N + 2, rows)
    outs = dedup_outs(zs.dev, N + 2)
    seen = []
    for _ in range(3):
        mo, _ = check_dedup(zs, srcs, deduper=dd, outs=outs, n_max=N + 2)
        seen.append(outs.pull())
    assert mo["count"][3] == 1 and mo["rep"][one.n + ORDER2.index(MIXED)] == one.n + ORDER2.index(MIXED)
    assert seen[0] == seen[1] == seen[2]
    dd.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_dedup_and_splice_in_one_captured_graph(fmt):
    """a dedup and the splice that consumes its d_pick, both executed for the first time inside a capture of the ctx stream, replayed twice"""
    import torch
    import ms_compress_amd as m
    f, B = FMTS[fmt], 4096
    base = R.buffers(B)
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        zs = Splices(ctx, f, B)
        n, dev = zs.rig[0].n, zs.dev
        N, rows = 2 * n, sum(x.nbt for x in zs.src)
        outs = dedup_outs(dev, N)
        dd = m.BlockDeduper(ctx, B, 2, N, rows)
        unique = sum(zs.rig[0].lens)
        nbt = N + unique // B
        sp = m.BlockSplicer(ctx, B, 2, N, nbt)
        so = zs.outputs(N, nbt)
        d_new, d_first, d_off, d_crc, d_len, d_st = so.tensors()
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        dd.dedup(dedup_views(zs.src, True), *outs.tensors())
        sp.splice(dedup_views(zs.src, True), outs["pick"], d_new, d_first, d_off, d_len, d_st, d_new_block_crc=d_crc, new_cap=zs.room)
    mo = D.model_dedup([x.model() for x in zs.src], B, True, n_res_total=N)
    picks = [(mo["pick"][2 * p], mo["pick"][2 * p + 1]) for p in range(N)]
    ms = S.model_splice([x.model() for x in zs.src], picks, B, nbt, zs.room)
    for k in range(2):
        with torch.cuda.stream(s):
            outs.reset()
            so.fill()
            g.replay()
        s.synchronize()
        outs.against(mo, exact=DEDUP_EXACT)
        new = zs.pull(so)
        zs.compare(new, ms, N, nbt)
        with torch.cuda.stream(s):
            zs.check_consequence(new, [base[r] for _, r in picks[: n - 1]] + [b""] * (n + 1), nbt)
    del g
    sp.close(); dd.close()
    zs.close()
    ctx.close()


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
    n = len(bufs0)
    rep, idx, picks, counts, st = m.blocks_dedup(cons, B, ctx=gpu_ctx)
    assert rep == expect_two_orders(n) and idx == rep and st == [0] * (2 * n)
    assert picks == [(0, r) for r in range(n - 1)] and counts[:2] == [n - 1, 2 * n] and counts[3] == 0
    new_packed, nfirst, noff, nlen, ncrc, status = m.blocks_splice(cons, picks, B, ctx=gpu_ctx)
    out, dst = m.blocks_decompress(f, new_packed, nfirst, noff, nlen, B, ctx=gpu_ctx, block_crc=ncrc)
    assert status == [0] * (n - 1) and dst == [0] * (n - 1) and out == bufs0[: n - 1]
    plain = m.blocks_dedup([c[:4] + (None,) for c in cons[:1]], B, ctx=gpu_ctx)
    assert plain[0] == list(range(n - 1)) + [EMPTY] and plain[3][:2] == [n - 1, n]
