"""GPU: mscomp_amd_parity_build and mscomp_amd_parity_rebuild against the model of tests/parity_model.py. Every output array is
sentinel-filled with guard entries behind it and compared whole; d_par and d_fix_packed are compared as images over FILL. The bytes behind
every stored row are the next row's and behind packed_len lies FILL, so a tail read that is not masked shows as wrong parity, not as a
fault. The header's consequence runs on the GPU from the calls' own device arrays: salvage, rebuild, salvage of the fix view, repair,
splice by extents -- byte for byte the healthy container. (The file's name: tests/test_gpu_parity.py is taken, by the tests that hold the
encoders to the reference.)"""
import ctypes as C

import numpy as np
import pytest

import parity_model as Y
import repair_model as P
from repair_model import GOOD, TABLE, CRC, SKIPPED

from blocks_rig import Container, Spliced, d64, flip, i32, memo, mixed, rand, soft, text, FMTS, FILL
from parity_rig import FixOuts, ParitySet, check_build, check_rebuild, fix_container, synthetic
from repair_rig import SalvageOuts, check_repair, check_salvage, rebuild, repair_outs

pytestmark = pytest.mark.gpu
B = 4096
SHAPES = [(1, 1), (3, 1), (4, 2), (5, 3), (255, 3)]


def bufs_4k():
    """raw rows (s = B), well-compressed rows, short last rows, a 1-byte resource and an empty one: 25 rows"""
    return [mixed(1, 9 * B + 50), soft(2, 7 * B + 5), b"", rand(3, 1), mixed(5, 5 * B + 17, period=3)]


def stored(h):
    nb = int(h.first[-1])
    return np.diff(np.asarray(h.off[: nb + 1], dtype=np.int64))


def input_conditions(h, k):
    """checked before anything runs: the rows start at 8 or more residues mod 16, and a group mixes a raw row with rows under 64 bytes"""
    nb, L = int(h.first[-1]), stored(h)
    G = (nb + k - 1) // k
    assert len(set((np.asarray(h.off[:nb]) % 16).tolist())) >= 8
    assert any((L[g::G] == h.B).any() and (L[g::G] < 64).sum() >= 2 for g in range(G)), "no group mixes a raw row with tiny ones"
    assert (L == h.B).sum() >= 5 and (L == 1).any() and 0 in h.lens


@pytest.fixture(scope="module")
def made(gpu_ctx):
    yield from memo()


def healthy_of(gpu_ctx, made, fmt):
    def make():
        h = Container.make(gpu_ctx, FMTS[fmt], B, bufs_4k())
        h.d_packed[h.plen:] = FILL                               # behind packed_len: not zeros, which would hide an unmasked tail
        assert int(h.first[-1]) == 25
        input_conditions(h, 5)
        return h
    return made(fmt, "healthy", make)


def parity_of(gpu_ctx, made, h, fmt, k, m):
    import ms_compress_amd as mm
    return made(fmt, k, m, lambda: mm.BlockParity(gpu_ctx, h.B, h.nbt, k, m))


def built_of(gpu_ctx, made, fmt, k, m):
    """(healthy container, its parity object, the healthy parity set and its length)"""
    h = healthy_of(gpu_ctx, made, fmt)
    pr = parity_of(gpu_ctx, made, h, fmt, k, m)

    def make():
        mo, pset = check_build(pr, h)
        assert mo["status"] == 0
        return pset, int(mo["par_off"][-1])
    return (h, pr) + made(fmt, k, m, "set", make)


def res_of(h, j):
    r = int(np.searchsorted(np.asarray(h.first[1:]), j, side="right"))
    return r, j - int(h.first[r])


def hit(oracle, h, rows):
    """the stored bytes with one byte of each row flipped -- in a compressed row a byte whose flip the reference refuses with defined
    behaviour --, and verdicts that name the rows"""
    packed, L = bytearray(h.packed), stored(h)
    ver = np.array([GOOD] * int(h.first[-1]) + [SKIPPED] * (h.nbt - int(h.first[-1])), dtype=np.uint32)
    for j in rows:
        r, kk = res_of(h, j)
        e = P.data_len(h, r, kk)
        at = int(h.off[j]) + min(5, int(L[j]) - 1) if L[j] == e else flip(oracle, h, j, e, False)   # (every row hit has stored bytes)
        packed[at] ^= 0xFF if L[j] == e else 0x01
        ver[j] = CRC if L[j] == e else 2
    return h.edited(packed=bytes(packed)), ver


# ---- build ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m", SHAPES)
@pytest.mark.parametrize("fmt", list(FMTS))
def test_build_against_the_model(gpu_ctx, made, fmt, k, m):
    """nb = 25: a multiple of k (1, 5) and not (3, 4); k >= nb gives G = 1. Exact capacity and 16 short; executed three times: plain,
    captured, replayed"""
    h, pr, pset, total = built_of(gpu_ctx, made, fmt, k, m)
    rows, room = pr.bound()
    assert (rows, room) == (m * ((h.nbt + k - 1) // k), m * ((h.nbt + k - 1) // k) * B) and total <= room
    mine = ParitySet(h.dev, h.nbt, k, m, room)
    for cap, st in ((total, Y.OK), (total - 16, Y.BUF), (total, Y.OK)):
        mo, _ = check_build(pr, h, pset=mine, par_cap=cap, what=(fmt, k, m, cap))
        assert mo["status"] == st and mo["head"] == [25, (25 + k - 1) // k, k, m]
    assert bytes(mine.d_par.cpu().numpy()[:total]) == bytes(pset.d_par.cpu().numpy()[:total])


def test_build_at_64k_and_the_column_tile_seam(gpu_ctx, made):
    """B = 65536, sixteen column tiles per group: a container of 6 rows with raw ones, and synthetic tables whose longest row puts plen
    on the seam of the first tile and one 16-byte step either side"""
    import ms_compress_amd as mm
    Bb, f = 65536, FMTS["xpress"]
    h = made("64k", lambda: Container.make(gpu_ctx, f, Bb, [rand(11, Bb + 77), soft(12, 2 * Bb + 1000), text(13, Bb - 3)]))
    h.d_packed[h.plen:] = FILL
    assert int(h.first[-1]) == 6 and (stored(h) == Bb).sum() >= 1
    for k, m in ((2, 3), (4, 2), (6, 1)):
        pr = mm.BlockParity(gpu_ctx, Bb, h.nbt, k, m)
        check_build(pr, h, what=("64k", k, m))
        pr.close()
    for plen in (4080, 4096, 4112, 8192, 8208):
        syn = synthetic(gpu_ctx, f, Bb, [plen - 3, 100, plen - 16, 1, 4000, 17], plen)   # (the first row at residue 3)
        pr = mm.BlockParity(gpu_ctx, Bb, 6, 6, 3)
        mo, _ = check_build(pr, syn, what=("seam", plen))
        assert mo["par_off"][1] == plen
        pr.close()


def test_build_empty_and_broken_tables(gpu_ctx, made):
    import ms_compress_amd as mm
    h = healthy_of(gpu_ctx, made, "xpress")
    pr = parity_of(gpu_ctx, made, h, "xpress", 4, 2)
    off = np.array(h.off, dtype=np.uint64)
    off[8] = off[7] - 1                                           # a decreasing entry: row 7 has length 0 and is never read; row 8 then spans two rows
    off[20] = h.plen + 9                                          # beyond packed_len: rows 19 and 20
    mo, _ = check_build(pr, h.edited(off=off), what="broken table")
    assert mo["row_len"][7] == 0 and mo["row_len"][19] == 0 and mo["row_len"][20] == 0 and mo["status"] == 0
    first = np.array(h.first, dtype=np.uint64)
    first[-1] = h.nbt + 1
    mo, _ = check_build(pr, h.edited(first=first), what="more rows than the table")
    assert mo["status"] == Y.ARG and mo["row_len"] is None
    mo, _ = check_build(pr, h, nbt=h.nbt - 1, what="a view of another table size")
    assert mo["status"] == Y.ARG
    none = h.edited(first=np.zeros(h.n + 1, dtype=np.uint64))       # an empty container: resources without a row
    mo, _ = check_build(pr, none, what="empty container")
    assert mo["status"] == 0 and mo["head"] == [0, 0, 4, 2] and mo["par_off"] == [0] * (2 * 7 + 1) and mo["row_len"] == [0] * h.nbt
    p0 = mm.BlockParity(gpu_ctx, B, 0, 4, 2)                       # no table at all: the header and the status alone
    assert p0.bound() == (0, 0)
    mo, pset0 = check_build(p0, none, nbt=0, what="n_blocks_table 0")
    assert mo["status"] == 0 and mo["head"] == [0, 0, 4, 2] and mo["par_off"] is None
    mo, _ = check_rebuild(p0, none, [], pset0, 0, nbt=0, what="n_blocks_table 0")
    assert mo["status"] == 0 and mo["count"] == [0] * 6 and mo["fix_off"] is None
    mo, _ = check_build(p0, h, nbt=0, what="n_blocks_table 0, a container with rows")
    assert mo["status"] == Y.ARG
    p0.close()


# ---- rebuild -------------------------------------------------------------------------------------------------------------------------------
def recipes(k, m, G):
    """name -> rows hit; G = 7 at (4, 2): group g has the rows g, g + 7, g + 14 and, below 4, g + 21"""
    return {"healthy": [], "one_per_group": [g + G * (g % 3) for g in range(G)], "m_of_one_group": [2, 2 + 2 * G][:m] if m < 3 else [2, 2 + G, 2 + 2 * G],
            "one_too_many": [2 + G * i for i in range(m + 1)] + [3, 4 + G], "longest": [4], "shortest": [4 + 2 * G]}


@pytest.mark.parametrize("name", ["healthy", "one_per_group", "m_of_one_group", "one_too_many", "longest", "shortest"])
@pytest.mark.parametrize("fmt", list(FMTS))
def test_rebuild_recipes(gpu_ctx, oracle, made, fmt, name):
    k, m = 4, 2
    h, pr, pset, total = built_of(gpu_ctx, made, fmt, k, m)
    rows = recipes(k, m, 7)[name]
    con, ver = hit(oracle, h, rows)
    L = stored(h)
    if name in ("longest", "shortest"):
        grp = L[4::7]                                             # group 4: a raw row, a compressed one and the 1-byte resource's
        assert L[rows[0]] == (grp.max() if name == "longest" else grp.min()) and grp.max() == B and grp.min() == 1
    mo, outs = check_rebuild(pr, con, ver, pset, total, what=(fmt, name))
    if name == "one_too_many":
        assert mo["status"] == Y.DATA and mo["unrecoverable"] == [2] and mo["rebuilt"] == [3, 11] and mo["count"][:4] == [5, 2, 3, 1]
    else:
        assert mo["status"] == 0 and mo["rebuilt"] == sorted(rows) and mo["count"][5] == int(L[rows].sum()) if rows else mo["count"] == [0] * 6
        fix = fix_container(h, outs, mo)
        for j in rows:
            assert fix.packed[int(fix.off[j]): int(fix.off[j + 1])] == h.packed[int(h.off[j]): int(h.off[j + 1])]


def test_rebuild_three_parities_and_a_burst(gpu_ctx, oracle, made):
    fmt = "lznt1"
    h, pr, pset, total = built_of(gpu_ctx, made, fmt, 5, 3)      # G = 5: three rows of group 1, two of group 3
    con, ver = hit(oracle, h, [1, 11, 21, 3, 18])
    mo, _ = check_rebuild(pr, con, ver, pset, total, what="three of a group")
    assert mo["status"] == 0 and mo["rebuilt"] == [1, 3, 11, 18, 21] and mo["used"] == {1: [0, 1, 2], 3: [0, 1]}
    h, pr, pset, total = built_of(gpu_ctx, made, fmt, 3, 1)      # G = 9: a burst of G consecutive rows costs every group one member
    con, ver = hit(oracle, h, list(range(5, 14)))
    mo, _ = check_rebuild(pr, con, ver, pset, total, what="a burst of G rows")
    assert mo["status"] == 0 and mo["rebuilt"] == list(range(5, 14)) and mo["count"][2] == 9
    con, ver = hit(oracle, h, list(range(5, 15)))                 # one row more: rows 5 and 14 share group 5
    mo, _ = check_rebuild(pr, con, ver, pset, total, what="a burst of G + 1 rows")
    assert mo["status"] == Y.DATA and mo["unrecoverable"] == [5] and len(mo["rebuilt"]) == 8
    h, pr, pset, total = built_of(gpu_ctx, made, fmt, 255, 3)    # one group of 25
    con, ver = hit(oracle, h, [0, 17, 24])
    mo, _ = check_rebuild(pr, con, ver, pset, total, what="k = 255")
    assert mo["status"] == 0 and mo["rebuilt"] == [0, 17, 24]
    h, pr, pset, total = built_of(gpu_ctx, made, fmt, 1, 1)      # k = 1: every row its own group, its parity a padded copy
    con, ver = hit(oracle, h, [4, 5, 18])
    mo, _ = check_rebuild(pr, con, ver, pset, total, what="k = 1")
    assert mo["status"] == 0 and mo["rebuilt"] == [4, 5, 18]


def test_rebuild_damaged_tables_parity_and_header(gpu_ctx, oracle, made):
    fmt, k, m, G = "xpress", 4, 2, 7
    h, pr, pset, total = built_of(gpu_ctx, made, fmt, k, m)
    outs = FixOuts(h.dev, h.nbt, h.plen + 64)
    ver = np.array([GOOD] * 25 + [SKIPPED] * (h.nbt - 25), dtype=np.uint32)
    off = np.array(h.off, dtype=np.uint64)
    off[11] = off[10]                                             # one entry: rows 10 and 11, groups 3 and 4
    v2 = ver.copy(); v2[10] = v2[11] = TABLE
    mo, _ = check_rebuild(pr, h.edited(off=off), v2, pset, total, outs=outs, what="an offset entry")
    assert mo["status"] == 0 and mo["rebuilt"] == [10, 11]
    mo, _ = check_rebuild(pr, h.edited(off=off), ver, pset, total, outs=outs, what="an offset entry the verdicts do not name")
    assert mo["rebuilt"] == [10, 11], "a row whose table length is not d_row_len is missing whatever its verdict"
    at = int(pset.host(total)["par_off"][2 * m]) + 21             # parity 0 of group 2
    bad = pset.damaged(par=[at])
    con, v1 = hit(oracle, h, [2 + G])
    mo, _ = check_rebuild(pr, con, v1, bad, total, outs=outs, what="a parity byte, e = 1")
    assert mo["status"] == 0 and mo["used"] == {2: [1]} and mo["count"][4] == 1
    con, v3 = hit(oracle, h, [2, 2 + G])
    mo, _ = check_rebuild(pr, con, v3, bad, total, outs=outs, what="a parity byte, e = 2")
    assert mo["status"] == Y.DATA and mo["unrecoverable"] == [2] and mo["rebuilt"] == []
    mo, _ = check_rebuild(pr, con, v3, pset.damaged(crc=[2 * m + 1]), total, outs=outs, what="a CRC word of the parity set")
    assert mo["status"] == Y.DATA and mo["count"][4] == 1
    mo, _ = check_rebuild(pr, con, v3, pset, total - 16, outs=outs, what="a parity set cut short")
    assert mo["count"][4] == 1 and mo["status"] == 0, "the last parity row ends beyond par_len: group 6 has nothing missing"
    other = pset.damaged()
    other.d_head = pset.d_head.clone()
    other.d_head[2] = 5                                           # parity of another shape
    mo, _ = check_rebuild(pr, con, v3, other, total, outs=outs, what="a header of another shape")
    assert mo["status"] == Y.DATA and mo["count"] == [0] * 6 and mo["fix_off"] == [0] * (h.nbt + 1)
    mo, _ = check_rebuild(pr, con, v3, pset, total, outs=outs, nbt=h.nbt - 1, what="a view of another table size")
    assert mo["status"] == Y.ARG
    mo, _ = check_rebuild(pr, con, v3, pset, total, outs=outs, what="room for both")
    need = mo["fix_off"][-1]
    cut, _ = check_rebuild(pr, con, v3, pset, total, outs=outs, fix_cap=need - 1, what="fix_cap one byte short")
    assert cut["status"] == Y.BUF and cut["fix_verdict"][2] == GOOD and cut["fix_verdict"][2 + G] == SKIPPED and cut["count"][1] == 2


# ---- the consequence -----------------------------------------------------------------------------------------------------------------------
def chain(oracle, h, pr, pset, total, con, mirrors=(), second="salvage"):
    """salvage, rebuild, salvage of the fix view with d_only (or d_fix_verdict in its place), repair, splice by extents"""
    ms, so, _ = check_salvage(oracle, h, con)
    mr, fo = check_rebuild(pr, con, ms["verdict"], pset, total, d_verdict=so.d_verdict)
    fix = fix_container(con, fo, mr)
    srcs, vers, d_vers = [con, fix], [ms["verdict"]], [so.d_verdict]
    if second == "salvage":
        mf, sf, _ = check_salvage(oracle, h, fix, only=ms["verdict"], what="the fix view")
        assert [int(v) for v in mf["verdict"][:25]] == [GOOD if j in mr["rebuilt"] else (SKIPPED if ms["verdict"][j] == GOOD else TABLE) for j in range(25)]
        vers.append(mf["verdict"]); d_vers.append(sf.d_verdict)
    else:
        vers.append(np.array(mr["fix_verdict"], dtype=np.uint32)); d_vers.append(fo.d_ver)
    for mir in mirrors:
        mv, sv, _ = check_salvage(oracle, h, mir, only=ms["verdict"], what="a real mirror")
        srcs.append(mir); vers.append(mv["verdict"]); d_vers.append(sv.d_verdict)
    ro, outs = check_repair(srcs, vers, d_verdicts=d_vers)
    rebuild(srcs, ro, outs, healthy=h)
    return mr, ro


@pytest.mark.parametrize("fmt", list(FMTS))
def test_the_consequence(gpu_ctx, oracle, made, fmt):
    k, m, G = 4, 2, 7
    h, pr, pset, total = built_of(gpu_ctx, made, fmt, k, m)
    for name in ("one_per_group", "m_of_one_group", "shortest"):
        con, _ = hit(oracle, h, recipes(k, m, G)[name])
        for second in ("salvage", "fix_verdict"):
            mr, ro = chain(oracle, h, pr, pset, total, con, second=second)
            assert mr["status"] == 0 and not any(ro["status"]) and ro["count"][0] == len(mr["rebuilt"]) > 0
    off = np.array(h.off, dtype=np.uint64)
    off[11] = off[10]
    mr, ro = chain(oracle, h, pr, pset, total, h.edited(off=off))
    assert mr["rebuilt"] == [10, 11] and not any(ro["status"])
    con, _ = hit(oracle, h, recipes(k, m, G)["one_too_many"])     # parity alone is not enough: a real mirror as the third source
    mr, ro = chain(oracle, h, pr, pset, total, con)
    assert mr["status"] == Y.DATA and sum(ro["lost"]) == 3
    mirror, _ = hit(oracle, h, [0, 3])                            # (damaged elsewhere, and in a row parity gives back)
    mr, ro = chain(oracle, h, pr, pset, total, con, mirrors=[mirror])
    assert not any(ro["status"]) and ro["count"][:2] == [5, 0]


def test_the_chain_in_one_captured_graph(oracle):
    """salvage, rebuild, salvage of the fix view, repair and splice by extents, all executed for the first time inside one capture of
    the ctx stream; the graph is replayed twice, the damage moved between the replays"""
    import torch
    import ms_compress_amd as m
    fmt, k, mm, G = "xpress", 4, 2, 7
    f = FMTS[fmt]
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        h = Container.make(ctx, f, B, bufs_4k())
        h.d_packed[h.plen:] = FILL
        builder, pr = m.BlockParity(ctx, B, h.nbt, k, mm), m.BlockParity(ctx, B, h.nbt, k, mm)
        mo, pset = check_build(builder, h)
        total = int(mo["par_off"][-1])
        fix_bk = m.BlockContainer(ctx, f, B, h.n, h.total)
        cases = [hit(oracle, h, [2, 16, 5])[0], hit(oracle, h, [0, 8, 13, 24])[0]]
        slot = h.edited(packed=h.packed)                          # rewritten in place below
        nb = int(h.first[-1])
        out_off, room = h.layout(h.lens)
        so = [SalvageOuts(h.dev, h.n, h.nbt, room) for _ in range(2)]
        d_ooff, d_caps = d64(out_off, h.dev), d64(h.lens, h.dev)
        fo = FixOuts(h.dev, h.nbt, h.plen + 64)
        fix_view = m.BlockParity.fix_view(slot.view(), fo.d_fix, fo.d_off, fix_len=fo.room)
        dd, sp = m.BlockDeduper.for_repair(ctx, B, 2, h.n, nb), m.BlockSplicer.for_extents(ctx, B, 2, h.n, nb, h.nbt)
        outs, built = repair_outs(h.dev, h.n, nb), Spliced(h.dev, h.n, h.nbt, h.plen + fo.room + 32, True)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        h.bk.salvage(slot.d_packed, slot.d_first, slot.d_boff, slot.d_len, so[0].d_out, d_ooff, d_caps, so[0].d_olen, so[0].d_bad, so[0].d_verdict, so[0].d_count,
                     so[0].d_st, d_block_crc=slot.d_crc, packed_len=slot.cap)
        fo.rebuild(pr, slot.view(False), so[0].d_verdict, pset, total)
        fix_bk.salvage(fo.d_fix, slot.d_first, fo.d_off, slot.d_len, so[1].d_out, d_ooff, d_caps, so[1].d_olen, so[1].d_bad, so[1].d_verdict, so[1].d_count,
                       so[1].d_st, d_block_crc=slot.d_crc, d_only=so[0].d_verdict, packed_len=fo.room)
        dd.repair([slot.view(), fix_view], [x.d_verdict for x in so], *outs.tensors())
        built.run(sp, [slot.view(), fix_view], outs["ext_first"], outs["ext"])
    for n, con in enumerate(cases):
        with torch.cuda.stream(s):
            slot.d_packed.copy_(con.d_packed)
            for x in so:
                x.reset()
            fo.reset(); outs.reset(); built.fill()
            g.replay()
        s.synchronize()
        ms = P.model_salvage(oracle, f, con.model(), B, h.total, h.lens)
        so[0].against(ms, out_off, B, ("primary, replay", n))
        mr = Y.model_rebuild(con.model(False), ms["verdict"], pset.host(total), B, k, mm, fo.room)
        fo.against(mr, ("rebuild, replay", n))
        assert mr["status"] == 0 and len(mr["rebuilt"]) == (3, 4)[n]
        fix = fix_container(con, fo, mr).edited(plen=fo.room)
        mf = P.model_salvage(oracle, f, fix.model(), B, h.total, h.lens, only=ms["verdict"])
        so[1].against(mf, out_off, B, ("fix view, replay", n))
        ro = P.model_repair([con.model(), fix.model()], [ms["verdict"], mf["verdict"]], B, h.n, nb)
        outs.against(ro, exact=("ext_first", "fixed", "lost", "count"), prefixes=("ext",))
        assert not any(ro["status"])
        built.against(P.model_rebuild([con.model(), fix.model()], ro, B, n_ext=nb, cap=built.room), "rebuilt, replay %d" % n)
        got = built.as_built()
        assert bytes(got["packed"][: h.plen]) == h.packed and np.array_equal(got["off"], h.off) and np.array_equal(got["crc"], h.crc)
    del g
    for x in (dd, sp, fix_bk, builder, pr, h):
        x.close()
    ctx.close()


# ---- refusals, two objects, the host conveniences --------------------------------------------------------------------------------------
def test_refusals_that_need_a_device(gpu_ctx, made):
    import ms_compress_amd as m
    h, pr, pset, total = built_of(gpu_ctx, made, "xpress", 4, 2)
    lib, fo = gpu_ctx.lib, FixOuts(h.dev, h.nbt, h.plen + 64)
    views = m.api._blocks_views([h.view(False)])
    p = lambda t: C.c_void_p(t.data_ptr())
    b = [p(pset.d_par), pset.room, p(pset.d_off), p(pset.d_crc), p(pset.d_rl), p(pset.d_head), p(pset.d_st)]
    before = bytes(pset.d_par.cpu().numpy())
    for i in (0, 2, 3, 4, 5, 6):
        args = list(b); args[i] = None
        assert lib.mscomp_amd_parity_build(pr._h, views, *args) == m.MSCOMP_ARG_ERROR, i
    assert lib.mscomp_amd_parity_build(pr._h, None, *b) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_parity_build(pr._h, views, C.c_void_p(pset.d_par.data_ptr() + 8), *b[1:]) == m.MSCOMP_ARG_ERROR, "a misaligned d_par"
    nofirst = m.api._blocks_views([h.view(False)]); nofirst[0].d_block_first = None
    assert lib.mscomp_amd_parity_build(pr._h, nofirst, *b) == m.MSCOMP_ARG_ERROR, "a view pack refuses"
    d_ver = i32(np.zeros(h.nbt, dtype=np.uint32), h.dev)
    r = [p(d_ver), p(pset.d_par), total, p(pset.d_off), p(pset.d_crc), p(pset.d_rl), p(pset.d_head), p(fo.d_fix), fo.room, p(fo.d_off), p(fo.d_ver), p(fo.d_count),
         p(fo.d_st)]
    for i in (0, 1, 3, 4, 5, 6, 7, 9, 10, 11, 12):
        args = list(r); args[i] = None
        assert lib.mscomp_amd_parity_rebuild(pr._h, views, *args) == m.MSCOMP_ARG_ERROR, i
    assert lib.mscomp_amd_parity_rebuild(pr._h, views, r[0], C.c_void_p(pset.d_par.data_ptr() + 4), *r[2:]) == m.MSCOMP_ARG_ERROR
    gpu_ctx.stream.synchronize()
    assert bytes(pset.d_par.cpu().numpy()) == before and int(pset.d_st.cpu()[0]) == 0, "a refused call writes nothing"
    with pytest.raises(m.MSCompError):
        m.BlockParity(gpu_ctx, B, 64, 0, 1)


def test_two_objects_used_alternately(gpu_ctx, oracle, made):
    h, pa, sa, ta = built_of(gpu_ctx, made, "xpress_huff", 4, 2)
    _, pb, sb, tb = built_of(gpu_ctx, made, "xpress_huff", 5, 3)
    ca, va = hit(oracle, h, [2, 16])
    cb, vb = hit(oracle, h, [1, 11, 21])
    oa, ob = FixOuts(h.dev, h.nbt, h.plen + 64), FixOuts(h.dev, h.nbt, h.plen + 64)
    for _ in range(3):                                            # plain, captured, replayed -- each between the other's
        ma, _ = check_rebuild(pa, ca, va, sa, ta, outs=oa, what="object a")
        mb, _ = check_rebuild(pb, cb, vb, sb, tb, outs=ob, what="object b")
        assert ma["rebuilt"] == [2, 16] and mb["rebuilt"] == [1, 11, 21]
        oa.against(ma, "object a, after b ran")
        check_build(pa, h, what="build a"); check_build(pb, h, what="build b")


def test_host_conveniences(gpu_ctx, oracle):
    import ms_compress_amd as m
    f = FMTS["xpress"]
    bufs = [text(7, 3 * B + 17), b"", mixed(8, 4 * B + 5), rand(9, 3000)]
    healthy = Container.via_host(gpu_ctx, f, B, bufs)
    par = m.blocks_parity(healthy.host(), B, 3, 2, ctx=gpu_ctx)
    mo = Y.model_build(healthy.model(False), B, 3, 2, 1 << 40)
    assert bytes(par[0]) == mo["set"]["par"] and list(par[1]) == mo["par_off"] and list(par[2]) == mo["par_crc"] and list(par[3]) == mo["row_len"]
    assert list(par[4]) == [10, 4, 3, 2]
    broken, _ = hit(oracle, healthy, [1, 5, 9, 6])                # rows 1, 5, 9 share group 1 of 4: one too many; row 6 comes back
    (packed, first, off, lens, crc), report = m.blocks_rebuild(f, broken.host(), par, B, ctx=gpu_ctx)
    assert report["rebuild_status"] == Y.DATA and report["rebuild_counts"][:4] == [4, 1, 2, 1] and report["counts"][:2] == [1, 3]
    broken, _ = hit(oracle, healthy, [1, 5, 6, 3])
    (packed, first, off, lens, crc), report = m.blocks_rebuild(f, broken.host(), par, B, ctx=gpu_ctx)
    assert report["rebuild_status"] == 0 and report["rebuild_counts"][:4] == [4, 4, 3, 0] and report["counts"][:2] == [4, 0] and not any(report["statuses"])
    assert bytes(packed) == healthy.packed and np.array_equal(off, healthy.off) and np.array_equal(crc, healthy.crc) and lens == healthy.lens
    mirror, _ = hit(oracle, healthy, [0])
    broken, _ = hit(oracle, healthy, [1, 5, 9, 6])
    (packed, first, off, lens, crc), report = m.blocks_rebuild(f, broken.host(), par, B, ctx=gpu_ctx, mirrors=[mirror.host()])
    assert report["rebuild_status"] == Y.DATA and report["counts"][:2] == [4, 0] and bytes(packed) == healthy.packed
    out, st = m.blocks_decompress(f, packed, first, off, lens, B, ctx=gpu_ctx, block_crc=crc)
    assert st == [0] * 4 and out == bufs
