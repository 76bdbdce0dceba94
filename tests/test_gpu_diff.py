"""GPU: mscomp_amd_deduper_diff against the model of tests/diff_model.py -- every entry of the seven outputs compared with sentinel-filled
arrays that are longer than the call may write (so a write behind the extents in use, or behind n_pair, fails) --, then the two splices the
header's consequence speaks of run on the GPU from the call's own device arrays: the delta lists over {new}, the patch lists over {base,
delta}; the rebuilt container is held to the extents model and, wherever every pair is accepted and the pairs name the new resources in
order, byte for byte to the new container. The containers are made by the GPU's blocks_compress / blocks_crc, their later versions by
blocks_write and blocks_resize."""
import numpy as np
import pytest

import blocks_model as M
import dedup_model as D
import diff_model as F
import read_model as R

from blocks_rig import Container, ListOuts, Spliced, d64, flipped, memo, rand, recipe, same_lists, soft, table_only, FMTS, BLOCKS, MIXED, POISONS, SENT

pytestmark = pytest.mark.gpu
NO = F.NO_BASE
EXACT, PREFIXES = ("delta_first", "patch_first", "changed", "count"), ("delta_ext", "patch_ext")


def Outs(dev, n, room):
    """the seven output arrays of a diff of n pairs within `room` new blocks, sentinel-filled and guarded"""
    outs = ListOuts(dev, {"delta_first": n + 1, "delta_ext": 4 * room, "patch_first": n + 1, "patch_ext": 4 * room, "changed": n, "count": 4}, n)
    outs.n, outs.room = n, room
    return outs


def d_pairs(pairs, dev):
    return d64(np.array([(int(a) & F.M64, int(b) & F.M64) for a, b in pairs], dtype=np.uint64), dev, 2)


def room_for(new, pairs):
    return sum(new.blocks(b) for _, b in pairs if 0 <= b < new.n)


def check_diff(base, new, pairs, with_crc=True, room=None, dd=None, outs=None, crc_views=None):
    """one call compared with the model, array for array; returns (model, Outs). crc_views: which of the two views bring checksums"""
    import ms_compress_amd as m
    ctx, B = new.ctx, new.B
    room = room_for(new, pairs) if room is None else room
    cb, cn = (with_crc, with_crc) if crc_views is None else crc_views
    deduper = dd or m.BlockDeduper.for_diff(ctx, B, len(pairs), room)
    outs = outs or Outs(new.dev, len(pairs), room)
    outs.reset()
    deduper.diff(base.view(cb), new.view(cn), d_pairs(pairs, new.dev), *outs.tensors())
    ctx.stream.synchronize()
    if dd is None:
        deduper.close()
    mo = F.model_diff(base.model(cb), new.model(cn), pairs, B, room, cb and cn)
    n = len(pairs)
    assert n == len(mo["status"]) == len(mo["changed"]) and len(mo["delta_first"]) == len(mo["patch_first"]) == n + 1 and len(mo["count"]) == 4
    outs.against(mo, exact=EXACT, prefixes=PREFIXES)
    return mo, outs


def rebuild(base, new, pairs, mo, outs, with_crc=True, same=None):
    """the header's consequence on the GPU, from the device arrays the diff left: the delta container out of {new}, then base + delta"""
    import ms_compress_amd as m
    ctx, B, n, room = new.ctx, new.B, len(pairs), outs.room
    md, mb = F.model_delta_and_patch(base.model(with_crc), new.model(with_crc), pairs, mo, B, room, with_crc)
    delta = Spliced(new.dev, n, room, len(md["packed"]) + 32, with_crc)
    built = Spliced(new.dev, n, room, len(mb["packed"]) + 32, with_crc)
    s1, s2 = m.BlockSplicer.for_extents(ctx, B, 1, n, room, room), m.BlockSplicer.for_extents(ctx, B, 2, n, room, room)
    delta.run(s1, [new.view(with_crc)], outs["delta_first"], outs["delta_ext"])
    built.run(s2, [base.view(with_crc), delta.view()], outs["patch_first"], outs["patch_ext"])
    ctx.stream.synchronize()
    s1.close(); s2.close()
    delta.against(md, "delta")
    built.against(mb, "rebuilt")
    assert len(md["packed"]) == mo["count"][2]
    same = (all(s == 0 for s in mo["status"]) and [b for _, b in pairs] == list(range(new.n))) if same is None else same
    if same:
        got = built.as_built()
        got["packed"] = got["packed"][: new.plen]
        F.same_container(got, new.model(with_crc)[:1] + (new.plen,) + new.model(with_crc)[2:], with_crc)
        assert int(got["off"][int(got["first"][new.n])]) == new.plen
    return md, mb


def identity(base, new):
    return F.default_pairs(base.model(), new.model())


@pytest.fixture(scope="module")
def cons(gpu_ctx):
    """containers by (format, block size, name), made once"""
    yield from memo()


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_empty_and_trivial_pairs(gpu_ctx, cons, fmt, B):
    bufs = [b"", recipe("text", 1, 1, -7, B), recipe("mixed", 2, 2, -7, B), recipe("random", 3, 3, -7, B), b""]
    con = cons(fmt, B, "trivial", lambda: Container.via_host(gpu_ctx, FMTS[fmt], B, bufs))
    for with_crc in (True, False):
        mo, outs = check_diff(con, con, identity(con, con), with_crc)                # identical: one base run per non-empty pair
        assert mo["count"] == [0, 6, 0, 0] and mo["patch_ext"] == [(0, 1, 0, 1), (0, 2, 0, 2), (0, 3, 0, 3)] and mo["delta_ext"] == []
        rebuild(con, con, identity(con, con), mo, outs, with_crc)
        pairs = [(NO, r) for r in range(5)]                                          # no base: one changed run
        mo, outs = check_diff(con, con, pairs, with_crc)
        assert mo["changed"] == [0, 1, 2, 3, 0] and mo["patch_ext"] == [(1, 1, 0, 1), (1, 2, 0, 2), (1, 3, 0, 3)] and mo["count"][2] == con.plen
        rebuild(con, con, pairs, mo, outs, with_crc)


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_local_changes(gpu_ctx, cons, fmt, B):
    bufs = [R.buffers(B)[MIXED], recipe("text", 4, 6, 33, B), recipe("random", 5, 1, 0, B)]
    base = cons(fmt, B, "local", lambda: Container.via_host(gpu_ctx, FMTS[fmt], B, bufs))
    one = lambda r, at: (r, at, bytes([bufs[r][at] ^ 0xFF]))
    new = base.written([one(0, 5), one(0, B + B // 2), one(0, 3 * B + 16)])            # the first, a middle and the last, short block
    mo, outs = check_diff(base, new, identity(base, new))
    assert mo["changed"] == [3, 0, 0] and mo["patch_ext"][:3] == [(1, 0, 0, 2), (0, 0, 2, 1), (1, 0, 2, 1)] and mo["count"][3] == 0
    rebuild(base, new, identity(base, new), mo, outs)
    alt = base.written([one(1, k * B + 9) for k in range(0, 7, 2)])                    # every other block: the extent-count maximum
    for with_crc in (True, False):
        mo, outs = check_diff(base, alt, identity(base, alt), with_crc)
        assert mo["changed"] == [0, 4, 0] and mo["patch_first"][2] - mo["patch_first"][1] == 7 == alt.blocks(1)
        rebuild(base, alt, identity(base, alt), mo, outs, with_crc)


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_length_changes(gpu_ctx, cons, fmt, B):
    bufs = [recipe("mixed", 10, 5, 0, B), recipe("random", 9, 3, 17, B), recipe("text", 8, 3, 17, B)]
    base = cons(fmt, B, "lengths", lambda: Container.via_host(gpu_ctx, FMTS[fmt], B, bufs))
    longer = base.resized([8 * B, 3 * B + 17, 3 * B + 17])                             # three blocks more
    mo, outs = check_diff(base, longer, identity(base, longer))
    assert mo["changed"] == [3, 0, 0] and mo["patch_ext"][:2] == [(0, 0, 0, 5), (1, 0, 0, 3)]
    rebuild(base, longer, identity(base, longer), mo, outs)
    shorter = base.resized([3 * B, 3 * B + 17, 3 * B + 17])                            # two blocks fewer: the base's are dropped
    mo, outs = check_diff(base, shorter, identity(base, shorter))
    assert mo["changed"] == [0, 0, 0] and mo["patch_ext"][0] == (0, 0, 0, 3)
    rebuild(base, shorter, identity(base, shorter), mo, outs)
    filled = base.resized([5 * B, 4 * B, 4 * B + 1])              # the short last block of the base is a full one now, with the same leading bytes
    for with_crc in (True, False):
        mo, outs = check_diff(base, filled, identity(base, filled), with_crc)
        assert mo["changed"] == [0, 1, 2] and mo["verdicts"][1] == [False, False, False, True] and mo["count"][3] == 0   # the data-length clause
        rebuild(base, filled, identity(base, filled), mo, outs, with_crc)
    mo, outs = check_diff(filled, base, identity(filled, base))                        # and back: the short block against the full one
    assert mo["changed"] == [0, 1, 1]
    rebuild(filled, base, identity(filled, base), mo, outs)


def test_tile_boundaries(gpu_ctx):
    """rows 1024 and 2048 of the numbering: runs of either kind that straddle them, runs that span a whole tile, a pair boundary on one"""
    B, f, T = 4096, FMTS["lznt1"], 1024
    rows = 2 * T + 5
    bufs = [soft(1, T * B), soft(2, (rows - 1) * B + 100)]
    base = Container.via_host(gpu_ctx, f, B, bufs)
    one = lambda r, k: (r, k * B + 11, bytes([bufs[r][k * B + 11] ^ 0xFF]))
    marks = {"both": list(range(1020, 1030)) + list(range(2040, 2050)), "early": list(range(10, 20)), "wide": list(range(1000, 2051)), "last": [rows - 1]}
    alone = [(1, 1)]
    for name, ks in marks.items():
        new = base.written([one(1, k) for k in ks])
        mo, outs = check_diff(base, new, alone)                                       # resource 1 alone: its block k is row k
        assert mo["changed"] == [len(ks)] and mo["count"][1] == rows
        rebuild(base, new, alone, mo, outs, same=False)
        if name == "both":
            assert mo["patch_ext"] == [(0, 1, 0, 1020), (1, 0, 0, 10), (0, 1, 1030, 1010), (1, 0, 10, 10), (0, 1, 2050, rows - 2050)]
            mo, outs = check_diff(base, new, identity(base, new))                     # behind resource 0: the pair boundary is row 1024
            assert mo["patch_first"] == [0, 1, 6] and mo["delta_ext"] == [(0, 1, 1020, 10), (0, 1, 2040, 10)]
            rebuild(base, new, identity(base, new), mo, outs)
        if name == "wide":
            assert mo["patch_ext"] == [(0, 1, 0, 1000), (1, 0, 0, 1051), (0, 1, 2051, 2)]
    mo, outs = check_diff(base, base, [(NO, 0), (1, 1), (NO, 0)], room=rows + 2 * T)      # one run per pair, each longer than a tile
    assert mo["patch_ext"] == [(1, 0, 0, T), (0, 1, 0, rows), (1, 2, 0, T)]
    rebuild(base, base, [(NO, 0), (1, 1), (NO, 0)], mo, outs)


def test_tile_scan_second_trip(gpu_ctx):
    """1024 * 1024 + 3 new rows, hand-made tables and no stored byte: the one-workgroup scan over the tiles' words takes a second trip of
    1024 tiles. Resource 0 has all rows but three, resource 1 the last three -- its first row is the first of the second trip's first
    tile --, and neither pair has a base: one changed run per pair. The patch extent of pair 1 starts at block 0 of the delta's
    resource 1 only if the count of changed blocks in front of the pair is carried over the trips with its running sum. The
    expectations are closed forms; the same construction at 2 * 1024 + 3 rows is held to the model first, which is what they rest on."""
    import ms_compress_amd as m
    B, pairs = 4096, [(NO, 0), (NO, 1)]

    def case(rows):
        want = {"delta_first": [0, 1, 2], "delta_ext": [0, 0, 0, rows - 3, 0, 1, 0, 3], "patch_first": [0, 1, 2], "patch_ext": [1, 0, 0, rows - 3, 1, 1, 0, 3],
                "changed": [rows - 3, 3], "count": [rows, rows, 0, 0], "status": [0, 0]}
        return table_only(gpu_ctx, B, [rows - 3, 3]), want

    con, want = case(2 * 1024 + 3)
    _, outs = check_diff(con, con, pairs)
    same_lists(outs, want)
    rows = 1024 * 1024 + 3
    con, want = case(rows)
    dd, outs = m.BlockDeduper.for_diff(gpu_ctx, B, 2, rows), Outs(con.dev, 2, rows)
    dd.diff(con.view(), con.view(), d_pairs(pairs, con.dev), *outs.tensors())
    gpu_ctx.stream.synchronize()
    dd.close()
    same_lists(outs, want)


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_compare_edges(gpu_ctx, cons, fmt, B):
    data = recipe("random", 9, 3, 17, B)
    base = cons(fmt, B, "edges", lambda: Container.via_host(gpu_ctx, FMTS[fmt], B, [data, data]))
    assert bytes(base.packed) == data + data                                          # every block is stored raw: the stored bytes are the data
    mid = B + B // 2
    plain = Container.via_host(gpu_ctx, FMTS[fmt], B, [flipped(data, mid), data])                # more than 16 bytes from both ends of block 1
    twin = Container.via_host(gpu_ctx, FMTS[fmt], B, [D.crc_twin(data, mid), data])
    assert (twin.crc == base.crc).all() and not (plain.crc == base.crc).all()
    pairs = [(0, 0), (1, 1)]
    mo, outs = check_diff(base, plain, pairs)
    assert mo["count"] == [1, 8, B, 0]                                                 # the checksum tells
    rebuild(base, plain, pairs, mo, outs)
    mo, outs = check_diff(base, twin, pairs)
    assert mo["count"] == [1, 8, B, 1] and mo["patch_ext"][:3] == [(0, 0, 0, 1), (1, 0, 0, 1), (0, 0, 2, 2)]   # only the bytes tell
    rebuild(base, twin, pairs, mo, outs)
    for views in ((True, False), (False, True), (False, False)):                       # a null d_block_crc in one view: no checksum takes part
        for new in (plain, twin):
            mo, outs = check_diff(base, new, pairs, crc_views=views)
            assert mo["count"] == [1, 8, B, 1]
    rebuild(base, twin, pairs, mo, outs, with_crc=False)


@pytest.mark.parametrize("fmt", list(FMTS))
def test_alignment(gpu_ctx, fmt):
    """sixteen copies of one resource of raw and compressed rows behind resources of 1 .. 16 bytes that put them at every residue mod 16,
    every copy against every copy; then a middle stored byte of a compressed row of one copy flipped"""
    B = 4096
    x = R.buffers(B)[MIXED]
    size = Container.via_host(gpu_ctx, FMTS[fmt], B, [x]).plen
    rs, bufs, at = np.random.RandomState(5), [], 0
    for k in range(16):
        pad = (k - at) % 16 or 16
        bufs += [rs.bytes(pad), x]
        at += pad + size
    many = Container.via_host(gpu_ctx, FMTS[fmt], B, bufs)
    starts = [int(many.off[int(many.first[2 * k + 1])]) for k in range(16)]
    assert sorted(s % 16 for s in starts) == list(range(16))
    pairs = [(2 * a + 1, 2 * b + 1) for a in range(16) for b in range(16)]
    mo, outs = check_diff(many, many, pairs)
    assert mo["count"] == [0, 4 * 256, 0, 0]
    j = int(many.first[2 * 6 + 1]) + 1                                                # row 1 of copy 6: text, stored compressed
    o0, o1 = int(many.off[j]), int(many.off[j + 1])
    assert 40 < o1 - o0 < B
    for where in (o0, (o0 + o1) // 2, o1 - 1):
        hurt = many.edited(packed=flipped(bytes(many.packed), where))
        mo, outs = check_diff(many, hurt, pairs)
        assert mo["count"] == [16, 4 * 256, 16 * (o1 - o0), 16] and [p for p, c in enumerate(mo["changed"]) if c] == [16 * a + 6 for a in range(16)]
        mo, outs = check_diff(hurt, many, pairs)
        assert mo["count"][3] == 16 and [p for p, c in enumerate(mo["changed"]) if c] == list(range(16 * 6, 16 * 7))


def test_one_block_of_many_pieces(gpu_ctx):
    """512 KiB stored raw, 32 pieces of 16 KiB, the two versions differ in the last piece alone"""
    B, f = 524288, FMTS["xpress"]
    data = rand(21, B) + rand(22, 100)
    base = Container.via_host(gpu_ctx, f, B, [data])
    assert bytes(base.packed) == data
    twin, plain = Container.via_host(gpu_ctx, f, B, [D.crc_twin(data, B - 3000)]), Container.via_host(gpu_ctx, f, B, [flipped(data, B - 3000)])
    mo, outs = check_diff(base, twin, [(0, 0)])
    assert mo["count"] == [1, 2, B, 1] and mo["patch_ext"] == [(1, 0, 0, 1), (0, 0, 1, 1)]
    rebuild(base, twin, [(0, 0)], mo, outs)
    mo, outs = check_diff(base, plain, [(0, 0)], with_crc=False)
    assert mo["count"] == [1, 2, B, 1]
    mo, outs = check_diff(base, plain, [(0, 0)])
    assert mo["count"] == [1, 2, B, 0]
    mo, outs = check_diff(base, base, [(0, 0)])
    assert mo["count"] == [0, 2, 0, 0]


@pytest.mark.parametrize("B", BLOCKS)
def test_refusals(gpu_ctx, cons, B):
    fmt = "xpress"
    good = cons(fmt, B, "recipes", lambda: Container.via_host(gpu_ctx, FMTS[fmt], B, R.buffers(B)))
    n, lens = good.n, good.lens
    falling = good.first.copy(); falling[3] = falling[4] + np.uint64(1)                # resource 3 by dedup's rule 1; resource 2 gets a row too many: its rule 2
    beyond = good.first.copy(); beyond[n] = np.uint64(good.nbt + 1)                    # the last, empty resource by dedup's rule 1
    odd = list(lens); odd[MIXED] += B                                                  # dedup's rule 2
    j = int(good.first[MIXED])
    past = good.off.copy(); past[j + 2:] = np.uint64(good.cap + 1)                     # dedup's rule 3: row 1 of MIXED ends beyond packed_len, and every row behind it
    back = good.off.copy(); back[j + 2] = back[j + 1] - np.uint64(1)                   # dedup's rule 3: a decreasing entry inside MIXED
    hurt = {"falling": (good.edited(first=falling), {3: M.ARG, 2: M.DATA}), "beyond": (good.edited(first=beyond), {n - 1: M.ARG}),
            "odd": (good.edited(lens=odd), {MIXED: M.DATA}), "past": (good.edited(off=past), {r: M.DATA for r in range(MIXED, n) if lens[r]}),
            "back": (good.edited(off=back), {MIXED: M.DATA})}
    pairs = [(r, r) for r in range(n)]
    for name, (con, bad) in hurt.items():
        for base, new in ((con, good), (good, con)):                                   # on either side
            mo, outs = check_diff(base, new, pairs)
            assert mo["status"] == [bad.get(r, 0) for r in range(n)], name
            assert [e[1] for e in mo["patch_ext"]] == [r for r in range(n) if lens[r] and r not in bad], name   # the neighbours stay what they are
            rebuild(base, new, pairs, mo, outs, same=False)
    # rule 1, and the order of the rules: indices before tables, dedup's rule 1 on either side before its rule 2 on either
    order = [(0, n), (n, 0), (NO, n), (NO, 1), (2, MIXED), (MIXED, 3), (3, MIXED), (MIXED, MIXED), (1 << 40, 1), (1, NO)]
    mo, outs = check_diff(hurt["falling"][0], hurt["odd"][0], order, room=64)
    assert mo["status"] == [M.ARG, M.ARG, M.ARG, 0, M.DATA, 0, M.ARG, M.DATA, M.ARG, M.ARG]
    rebuild(hurt["falling"][0], hurt["odd"][0], order, mo, outs, same=False)
    # a base row at or behind n_b is dropped, not judged
    cut = Container.via_host(gpu_ctx, FMTS[fmt], B, [R.buffers(B)[MIXED][:B]])
    mo, outs = check_diff(hurt["back"][0], cut, [(MIXED, 0)])
    assert mo["status"] == [0] and mo["patch_ext"] == [(0, MIXED, 0, 1)]
    # rule 3: room exhausted at a middle pair; the pairs without blocks behind it pass
    mo, outs = check_diff(good, good, pairs, room=6)
    assert mo["status"] == [0, 0, 0, 0, 0] + [M.ARG] * (n - 6) + [0] and mo["count"][1] == 5
    rebuild(good, good, pairs, mo, outs, same=False)


def test_wrong_kind_nulls_and_no_pairs(gpu_ctx, cons):
    import torch
    import ms_compress_amd as m
    B = 4096
    good = cons("xpress", B, "recipes", lambda: Container.via_host(gpu_ctx, FMTS["xpress"], B, R.buffers(B)))
    n, dev = good.n, good.dev
    pairs = [(r, r) for r in range(n)]
    room = room_for(good, pairs)
    outs = Outs(dev, n, room)
    full = (d_pairs(pairs, dev),) + outs.tensors()
    # the wrong kind of deduper, both ways
    dd = m.BlockDeduper(gpu_ctx, B, 2, 2 * n, 2 * good.nbt)
    with pytest.raises(m.MSCompError) as e:
        dd.diff(good.view(), good.view(), *full)
    assert e.value.status == m.MSCOMP_ARG_ERROR
    dd.close()
    df = m.BlockDeduper.for_diff(gpu_ctx, B, n, room)
    rep = torch.full((2 * n,), SENT, dtype=torch.int64, device=dev)
    with pytest.raises(m.MSCompError) as e:
        df.dedup([good.view(), good.view()], rep, rep.clone(), torch.full((4 * n,), SENT, dtype=torch.int64, device=dev), outs["count"], outs.status)
    assert e.value.status == m.MSCOMP_ARG_ERROR
    # every array missing in turn, a view without a table, a view without stored bytes, no views at all
    for k in range(len(full)):
        with pytest.raises(m.MSCompError) as e:
            df.diff(good.view(), good.view(), *(full[:k] + (None,) + full[k + 1:]))
        assert e.value.status == m.MSCOMP_ARG_ERROR, k
    v = good.view()
    for broken in (v[:1] + (None,) + v[2:], v[:2] + (None,) + v[3:], v[:3] + (None,) + v[4:], (None,) + v[1:]):
        for a, b in ((broken, v), (v, broken)):
            with pytest.raises(m.MSCompError) as e:
                df.diff(a, b, *full)
            assert e.value.status == m.MSCOMP_ARG_ERROR
    views = m.api._blocks_views([v, v])
    import ctypes as C
    ptrs = [C.c_void_p(t.data_ptr()) for t in full]
    assert gpu_ctx.lib.mscomp_amd_deduper_diff(df._h, None, C.byref(views[1]), *ptrs) == m.MSCOMP_ARG_ERROR
    assert gpu_ctx.lib.mscomp_amd_deduper_diff(df._h, C.byref(views[0]), None, *ptrs) == m.MSCOMP_ARG_ERROR
    torch.cuda.synchronize()
    assert outs.untouched() and set(rep.cpu().tolist()) == {SENT}
    df.close()
    # no pairs: the counts and entry 0 of the two running counts; d_count alone is required
    for room0 in (0, 7):
        mo, o0 = check_diff(good, good, [], room=room0)
        assert mo["count"] == [0, 0, 0, 0] and mo["delta_first"] == [0] and mo["patch_first"] == [0]
    d0 = m.BlockDeduper.for_diff(gpu_ctx, B, 0, 0)
    cnt = torch.full((4,), SENT, dtype=torch.int64, device=dev)
    d0.diff(good.view(), good.view(), None, None, None, None, None, None, cnt, None)
    gpu_ctx.stream.synchronize()
    assert cnt.cpu().tolist() == [0, 0, 0, 0]
    d0.close()
    # pairs, and no room for a block: the pairs without blocks are accepted
    mo, _ = check_diff(good, good, pairs, room=0)
    assert mo["status"] == [0 if not x else M.ARG for x in good.lens] and mo["count"] == [0, 0, 0, 0]


def busy_case(gpu_ctx, cons, fmt, B=4096):
    """a base and a new version with every kind of verdict in them: runs of both kinds, a refuted block, a longer and a shorter resource, a
    resource without a base, and -- from the pairs -- a refused pair between accepted ones"""
    bufs = [R.buffers(B)[MIXED], recipe("random", 9, 3, 17, B), recipe("text", 4, 6, 33, B), recipe("mixed", 10, 5, 0, B)]
    base = cons(fmt, B, "busy0", lambda: Container.via_host(gpu_ctx, FMTS[fmt], B, bufs))

    def make():
        one = lambda r, at: (r, at, bytes([bufs[r][at] ^ 0xFF]))
        twin = D.crc_twin(bufs[1], B + 77)
        step = base.written([one(0, 3 * B + 1), one(2, 9), one(2, 4 * B + 9), (1, B + 77, twin[B + 77: B + 82])])
        return step.resized([step.lens[0], step.lens[1], step.lens[2] + 2 * B, 2 * B + 5])
    new = cons(fmt, B, "busy1", make)
    pairs = [(0, 0), (1, 1), (7, 2), (2, 2), (3, 3), (NO, 1), (3, 0)]
    return base, new, pairs


@pytest.mark.parametrize("fmt", list(FMTS))
def test_three_executions_are_identical(gpu_ctx, cons, fmt):
    import ms_compress_amd as m
    base, new, pairs = busy_case(gpu_ctx, cons, fmt)
    room = room_for(new, pairs) + 3
    dd = m.BlockDeduper.for_diff(gpu_ctx, base.B, len(pairs), room)
    outs = Outs(base.dev, len(pairs), room)
    seen = []
    for _ in range(3):
        mo, _ = check_diff(base, new, pairs, room=room, dd=dd, outs=outs)
        seen.append(outs.pull())
    assert mo["count"][3] == 1 and mo["status"][2] == M.ARG and mo["changed"][1] == 1 and mo["count"][0] > 8
    assert seen[0] == seen[1] == seen[2]
    rebuild(base, new, pairs, mo, outs, same=False)
    dd.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_scratch_contract(gpu_ctx, cons, fmt):
    """the scheme of tests/test_gpu_scratch.py: what an execution reads from the scratch it has written itself, and no pass touches the slack"""
    import ms_compress_amd as m
    base, new, pairs = busy_case(gpu_ctx, cons, fmt)
    room = room_for(new, pairs) + 3
    dd = m.BlockDeduper.for_diff(gpu_ctx, base.B, len(pairs), room)
    outs = Outs(base.dev, len(pairs), room)
    check_diff(base, new, pairs, room=room, dd=dd, outs=outs)
    first = outs.pull()
    rep = m.api.scratch_report(dd, 0)
    assert list(rep) == ["tab"] and rep["tab"][0] == 32 * len(pairs) + 4 * room + 64 * ((room + 1023) // 1024) + 72 and rep["tab"][1] >= rep["tab"][0]
    for byte in POISONS:
        assert m.api.scratch_poison(dd, byte) == 1                                     # the whole buffer, under the deduper's kind
        check_diff(base, new, pairs, room=room, dd=dd, outs=outs)
        assert outs.pull() == first, "after poison 0x%02X" % byte
        rep = m.api.scratch_report(dd, byte)
        assert rep["tab"][2] == 0, ("slack bytes touched", byte, rep)
    assert m.api.scratch_poison(dd, 0x11, slack_only=True) == (1 if rep["tab"][1] > rep["tab"][0] else 0)
    assert m.api.scratch_report(dd, 0x22)["tab"][2] == rep["tab"][1] - rep["tab"][0]   # the instrument itself: other slack bytes are reported
    dd.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_diff_and_both_splices_in_one_captured_graph(fmt):
    """diff, the delta splice and the patch splice, all executed for the first time inside one capture of the ctx stream; the graph is then
    replayed on the first pair of containers and on a second pair of the same bounds, loaded into the same device arrays"""
    import torch
    import ms_compress_amd as m
    f, B = FMTS[fmt], 4096
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        bufs = [R.buffers(B)[MIXED], recipe("text", 4, 6, 33, B), recipe("random", 5, 2, 0, B)]
        other = [recipe("mixed", 31, 3, 17, B), recipe("zeros", 32, 6, 33, B), recipe("text", 33, 2, 0, B)]
        one = lambda src, r, at: (r, at, bytes([src[r][at] ^ 0xFF]))
        base1 = Container.via_host(ctx, f, B, bufs)
        new1 = base1.written([one(bufs, 0, 7), one(bufs, 1, 2 * B + 1), one(bufs, 1, 3 * B + 1)])
        base2 = Container.via_host(ctx, f, B, other)
        new2 = base2.written([one(other, 1, 9), one(other, 2, B), one(other, 0, 3 * B + 2)])
        cap = max(c.plen for c in (base1, new1, base2, new2)) + 100
        slots = [Container.from_host(ctx, f, B, c.packed, c.first, c.off, c.lens, c.crc, cap=cap) for c in (base1, new1)]
        pairs = identity(base1, new1)
        n, room = len(pairs), room_for(new1, pairs)
        outs = Outs(base1.dev, n, room)
        dd = m.BlockDeduper.for_diff(ctx, B, n, room)
        s1, s2 = m.BlockSplicer.for_extents(ctx, B, 1, n, room, room), m.BlockSplicer.for_extents(ctx, B, 2, n, room, room)
        delta, built = Spliced(base1.dev, n, room, cap, True), Spliced(base1.dev, n, room, cap, True)
        d_pair = d_pairs(pairs, base1.dev)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        dd.diff(slots[0].view(), slots[1].view(), d_pair, *outs.tensors())
        delta.run(s1, [slots[1].view()], outs["delta_first"], outs["delta_ext"])
        built.run(s2, [slots[0].view(), delta.view()], outs["patch_first"], outs["patch_ext"])
    for k, (base, new) in enumerate(((base1, new1), (base2, new2), (base1, new1))):
        assert base.lens == base1.lens and new.nbt == new1.nbt
        with torch.cuda.stream(s):
            for slot, con in zip(slots, (base, new)):
                slot.d_packed.fill_(0x3C); slot.d_packed[: con.plen] = con.d_packed[: con.plen]
                slot.d_first.copy_(con.d_first); slot.d_boff.copy_(con.d_boff); slot.d_crc.copy_(con.d_crc)
            outs.reset(); delta.fill(); built.fill()
            g.replay()
        s.synchronize()
        held = [Container.from_host(ctx, f, B, c.packed + b"\x3C" * (cap - c.plen), c.first, c.off, c.lens, c.crc) for c in (base, new)]   # what the slots hold, as the model reads it
        mo = F.model_diff(held[0].model(), held[1].model(), pairs, B, room, True)
        outs.against(mo, exact=EXACT, prefixes=PREFIXES)
        assert mo["count"][0] == 3, k
        md, mb = F.model_delta_and_patch(held[0].model(), held[1].model(), pairs, mo, B, room, True)
        delta.against(md, "delta, replay %d" % k)
        built.against(mb, "rebuilt, replay %d" % k)
        rebuilt = built.as_built()
        rebuilt["packed"] = rebuilt["packed"][: new.plen]
        F.same_container(rebuilt, new.model()[:1] + (new.plen,) + new.model()[2:])
    del g
    for h in (dd, s1, s2):
        h.close()
    ctx.close()


def test_host_convenience(gpu_ctx):
    import ms_compress_amd as m
    f, B = 3, 4096
    old = [recipe("text", 41, 3, 17, B), recipe("mixed", 42, 2, 0, B), b"", recipe("random", 43, 1, 5, B)]
    new = [flipped(old[0], B + 1), old[1] + recipe("text", 44, 1, 9, B), b"", old[3], recipe("text", 45, 2, 1, B)]
    cons = []
    for bufs in (old, new):
        packed, first, off, st = m.blocks_compress(f, bufs, B, ctx=gpu_ctx)
        bcrc, _ = m.blocks_crc(f, bufs, B, ctx=gpu_ctx)
        cons.append((packed, first, off, [len(b) for b in bufs], bcrc))
    delta_res, patch_res, changed, counts, st = m.blocks_diff(cons[0], cons[1], B, ctx=gpu_ctx)
    assert st == [0] * 5 and changed == [1, 2, 0, 0, 3] and counts[:2] == [6, 13] and counts[3] == 0
    assert delta_res == [[(0, 0, 1, 1)], [(0, 1, 2, 2)], [], [], [(0, 4, 0, 3)]]
    assert patch_res == [[(0, 0, 0, 1), (1, 0, 0, 1), (0, 0, 2, 2)], [(0, 1, 0, 2), (1, 1, 0, 2)], [], [(0, 3, 0, 2)], [(1, 4, 0, 3)]]
    delta, patch2, changed2, counts2, st2 = m.blocks_delta(cons[0], cons[1], B, ctx=gpu_ctx)
    assert (patch2, changed2, counts2, st2) == (patch_res, changed, counts, st)
    assert len(delta[0]) == counts[2] < len(cons[1][0]) and [int(x) for x in delta[1]] == [0, 1, 3, 3, 3, 6]
    packed, first, off, lens, crc, status = m.blocks_patch(cons[0], delta, patch_res, B, ctx=gpu_ctx)
    assert status == [0] * 5 and lens == cons[1][3]
    assert bytes(packed) == bytes(cons[1][0]) and (first == cons[1][1]).all() and (off == cons[1][2]).all() and (crc == cons[1][4]).all()
    out, dst = m.blocks_decompress(f, packed, first, off, lens, B, ctx=gpu_ctx, block_crc=crc)
    assert dst == [0] * 5 and out == new
    only = m.blocks_diff(cons[0][:4] + (None,), cons[1], B, pairs=[(None, 3), (3, 3), (9, 0)], ctx=gpu_ctx)     # explicit pairs, no checksums
    assert only[2] == [2, 0, 0] and only[4] == [0, 0, m.MSCOMP_ARG_ERROR] and only[1][:2] == [[(1, 0, 0, 2)], [(0, 3, 0, 2)]]
