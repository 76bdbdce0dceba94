"""GPU: mscomp_amd_blocks_salvage and mscomp_amd_deduper_repair against the models of tests/repair_model.py. Every output array is
sentinel-filled and guarded, and the whole d_out image is compared: data in good rows, zeros in bad rows, FILL everywhere else and in every
unjudged row. After a repair the splice by extents runs on the GPU from the call's own device arrays; the rebuilt container is held to
the extents model and, where nothing is lost, byte for byte to the undamaged container. The containers are made by the GPU's compress and
crc (Container.make); damage is data only -- flipped stored bytes, table entries and CRC words, the bytes chosen by blocks_rig.flip among
those the reference decodes with defined behaviour."""
import numpy as np
import pytest

import read_model as R
import repair_model as P
from repair_model import GOOD, TABLE, DECODE, CRC, SKIPPED

from blocks_rig import Container, Spliced, d64, i32, memo, recipe, same_lists, table_only, text, FMTS, FILL, POISONS, SENT, SENT32, ST_FILL
from repair_rig import SalvageOuts, check_repair, check_salvage, damaged, rebuild, repair_outs

pytestmark = pytest.mark.gpu
B = 4096


@pytest.fixture(scope="module")
def cons(gpu_ctx):
    """containers by (format, name), made once"""
    yield from memo()


def healthy_of(gpu_ctx, cons, fmt, B=B):
    return cons(fmt, B, "buffers", lambda: Container.make(gpu_ctx, FMTS[fmt], B, R.buffers(B)))


@pytest.mark.parametrize("fmt", list(FMTS))
def test_healthy_container_is_all_good(gpu_ctx, oracle, cons, fmt):
    import torch
    h = healthy_of(gpu_ctx, cons, fmt)
    nb = int(h.first[-1])
    for crc in (True, False):
        mo, outs, out_off = check_salvage(oracle, h, h, crc=crc)
        assert (mo["verdict"][:nb] == GOOD).all() and mo["count"] == [nb, 0, 0, 0] and mo["status"] == [0] * h.n
        got = outs.pull()["image"]
        for r, o in enumerate(out_off):
            assert bytes(got[o: o + h.lens[r]]) == h.bufs[r]
        d_out = torch.full_like(outs.d_out, FILL)                  # ... and what decompress writes at the same places
        d_olen, d_st = torch.zeros(h.n, dtype=torch.int64, device=h.dev), torch.zeros(h.n, dtype=torch.int32, device=h.dev)
        h.bk.decompress(h.d_packed, h.d_first, h.d_boff, h.d_len, d_out, d64(out_off, h.dev), d64(h.lens, h.dev), d_olen, d_st, packed_len=h.plen)
        gpu_ctx.stream.synchronize()
        assert not d_st.cpu().numpy().any() and torch.equal(d_out, outs.d_out)


@pytest.mark.parametrize("name", list(P.RECIPES))
@pytest.mark.parametrize("fmt", list(FMTS))
def test_damage_recipes(gpu_ctx, oracle, cons, fmt, name):
    h = healthy_of(gpu_ctx, cons, fmt)
    edits = P.RECIPES[name](h, oracle)
    con = damaged(h, edits)
    for crc in (True, False):
        mo, _, _ = check_salvage(oracle, h, con, caps=edits.get("caps"), crc=crc, what=(name, crc))
        assert not crc or any(v in P.BAD for v in mo["verdict"]), "the recipe damages something"
    if name == "refused":
        assert {P.ARG, P.DATA, P.BUF} <= set(mo["status"])


@pytest.mark.parametrize("fmt", list(FMTS))
def test_only_mask(gpu_ctx, oracle, cons, fmt):
    h = healthy_of(gpu_ctx, cons, fmt)
    primary = damaged(h, P.r_everything(h, oracle))
    whole, _, _ = check_salvage(oracle, h, primary)
    nothing, outs, _ = check_salvage(oracle, h, primary, only=np.zeros(h.nbt, dtype=np.uint32), what="all good: nothing judged")
    assert nothing["count"] == [0, 0, 0, 0] and (outs.pull()["image"] == FILL).all()
    mirror = damaged(h, {"crc": P._crc(h, [P.row(h, P.ZEROS5, 2), P.row(h, P.SHORT_TEXT)])})   # damaged where the primary is good: not looked at
    masked, _, _ = check_salvage(oracle, h, mirror, only=whole["verdict"], what="the primary's verdicts")
    assert masked["count"] == [whole["count"][1], 0, 0, 0] and masked["status"] == [0] * h.n
    behind = whole["verdict"].copy()
    behind[int(h.first[-1]):] = np.resize([GOOD, DECODE, CRC, TABLE], h.nbt - int(h.first[-1]))   # words behind the real rows: ignored
    again, _, _ = check_salvage(oracle, h, mirror, only=behind, what="a mask with words behind the real rows")
    assert np.array_equal(again["verdict"], masked["verdict"]) and again["count"] == masked["count"]


def test_zero_fill_pieces_at_64k(gpu_ctx, oracle, cons):
    """B = 65536: a bad block of 65536 bytes (four pieces) and one of 16385 (a piece and one byte), a good resource on either side"""
    Bb, fmt = 65536, "xpress"
    bufs = [text(41, 100), text(42, Bb + 16385), text(43, Bb + 7)]
    h = cons(fmt, Bb, "pieces", lambda: Container.make(gpu_ctx, FMTS[fmt], Bb, bufs))
    con = damaged(h, {"packed": P._flips(h, oracle, [(1, 0, False), (1, 1, False)])})
    mo, _, _ = check_salvage(oracle, h, con)
    assert [v for v in mo["verdict"][:5]] == [GOOD, DECODE, DECODE, GOOD, GOOD] and mo["count"] == [5, 2, Bb + 16385, 1]


def test_output_offsets_at_every_residue(gpu_ctx, oracle, cons):
    fmt = "lznt1"
    bufs = [text(50 + q, B + 100 + q) for q in range(16)]
    h = cons(fmt, B, "residues", lambda: Container.make(gpu_ctx, FMTS[fmt], B, bufs))
    con = damaged(h, {"packed": P._flips(h, oracle, [(q, 0, False) for q in range(16)])})
    mo, _, out_off = check_salvage(oracle, h, con, residues=list(range(16)))
    assert sorted(o % 16 for o in out_off) == list(range(16)) and mo["bad"] == [1] * 16


def salvaged_case(oracle, h, recipes, crc=True):
    """the containers of a repair case, each salvaged on the GPU as blocks_repair does it: (containers, verdict arrays of the models)"""
    srcs = [damaged(h, r(h, oracle)) for r in recipes]
    verdicts = []
    for i, con in enumerate(srcs):
        only = verdicts[0] if i and con.lens == srcs[0].lens else None
        verdicts.append(check_salvage(oracle, h, con, crc=crc, only=only, what=("source", i))[0]["verdict"])
    return srcs, verdicts


@pytest.mark.parametrize("fmt", list(FMTS))
def test_repair_against_the_model(gpu_ctx, oracle, cons, fmt):
    h = healthy_of(gpu_ctx, cons, fmt)
    srcs, verdicts = salvaged_case(oracle, h, P.REPAIR_CASE)
    mo, outs = check_repair(srcs, verdicts)
    assert mo["count"][1] == 3 and mo["choice"][P.TEXT][1] == (0, True) and mo["choice"][P.RANDOM3][1] == (2, False) and mo["choice"][P.MIXED5][3] == (0, True)
    rebuild(srcs, mo, outs, healthy=h)
    srcs, verdicts = salvaged_case(oracle, h, (P.r_mendable, lambda s, o: {}))      # nothing lost: the undamaged container, byte for byte
    mo, outs = check_repair(srcs, verdicts)
    assert mo["status"] == [0] * h.n and mo["count"][:2] == [6, 0]
    rebuild(srcs, mo, outs, healthy=h)
    srcs, verdicts = salvaged_case(oracle, h, P.REPAIR_CASE, crc=False)              # without checksums
    mo, outs = check_repair(srcs, verdicts, with_crc=False)
    rebuild(srcs, mo, outs, with_crc=False)


def test_run_tiles_change_at_their_seams(gpu_ctx, cons):
    """one resource of 2 100 rows, small stored bytes: the choice changes at rows 1023 | 1024 and 2047 | 2048 and, in a second call, at
    every row around the first seam with lost rows on both sides of the second; the verdicts are the call's input, written here"""
    rows, fmt = 2100, "xpress"
    data = b"".join(text(70 + k, B) if k % 97 == 0 else bytes(B) for k in range(rows))
    h = cons(fmt, B, "long", lambda: Container.make(gpu_ctx, FMTS[fmt], B, [text(69, 33), data, text(68, B + 1)]))
    f = int(h.first[1])
    good = np.full(h.nbt, SKIPPED, dtype=np.uint32)
    good[: int(h.first[-1])] = GOOD
    v0 = good.copy(); v0[f + 1024: f + 2048] = DECODE
    mo, outs = check_repair([h, h], [v0, good])
    assert mo["ext"][1:4] == [(0, 1, 0, 1024), (1, 1, 1024, 1024), (0, 1, 2048, 52)] and mo["count"][:2] == [1024, 0]
    rebuild([h, h], mo, outs, healthy=h)
    v0, v1 = good.copy(), good.copy()
    v0[f + 1000: f + 1100: 2] = CRC; v0[f + 2046: f + 2050] = TABLE; v1[f + 2047: f + 2049] = DECODE
    mo, outs = check_repair([h, h], [v0, v1])
    assert mo["lost"] == [0, 2, 0] and mo["fixed"] == [0, 52, 0] and mo["ext_first"][2] - mo["ext_first"][1] == 105
    rebuild([h, h], mo, outs)


def test_tile_scan_second_trip(gpu_ctx):
    """1024 * 1024 + 3 rows, hand-made tables and no stored byte: the one-workgroup scan over the tiles' words takes a second trip of
    1024 tiles. One resource, every verdict GOOD but a DECODE stretch of four rows that straddles row 1024 * 1024 -- the first row of the
    second trip's first tile --, mended by one mirror: three extents, whose place in the list and whose first rows are the running sum
    and the running maximum carried from the first trip. The expectations are closed forms; the same construction at 2 * 1024 + 3 rows
    is held to the model first, which is what the closed forms rest on."""
    import ms_compress_amd as m

    def case(rows):
        seam = rows - 3
        good = np.full(rows, GOOD, dtype=np.uint32)
        v0 = good.copy(); v0[seam - 2: seam + 2] = DECODE
        want = {"ext_first": [0, 3], "ext": [0, 0, 0, seam - 2, 1, 0, seam - 2, 4, 0, 0, seam + 2, 1], "fixed": [4], "lost": [0],
                "count": [4, 0, 0, 0], "status": [0]}
        return table_only(gpu_ctx, B, [rows]), [v0, good], want

    con, verdicts, want = case(2 * 1024 + 3)
    _, outs = check_repair([con, con], verdicts)
    same_lists(outs, want)
    rows = 1024 * 1024 + 3
    con, verdicts, want = case(rows)
    dd, outs = m.BlockDeduper.for_repair(gpu_ctx, B, 2, 1, rows), repair_outs(con.dev, 1, rows)
    dd.repair([con.view(), con.view()], [i32(v, con.dev) for v in verdicts], *outs.tensors())
    gpu_ctx.stream.synchronize()
    dd.close()
    same_lists(outs, want)


def test_more_resources_than_one_scan_pass(gpu_ctx, oracle, cons):
    """1 030 tiny resources: the 1024-thread resource scans of salvage and of repair's seed take a second pass"""
    n, fmt = 1030, "lznt1"
    bufs = [text(100 + r, 1 + r % 37) if r % 3 else bytes(40 + r % 5) for r in range(n)]
    h = cons(fmt, B, "many", lambda: Container.make(gpu_ctx, FMTS[fmt], B, bufs))
    hit = (5, 1023, 1024, 1029)
    crc = np.array(h.crc, dtype=np.uint32)
    for r in hit:
        crc[P.row(h, r)] ^= 1
    off = np.array(h.off, dtype=np.uint64)
    off[P.row(h, 1027) + 1] = off[P.row(h, 1027)]                  # s = 0; the block behind it then holds both
    con = damaged(h, {"crc": crc, "off": off})
    mo, _, _ = check_salvage(oracle, h, con)
    assert [r for r, b in enumerate(mo["bad"]) if b] == [5, 1023, 1024, 1027, 1028, 1029]
    mirror = check_salvage(oracle, h, h, only=mo["verdict"])[0]
    ro, outs = check_repair([con, h], [mo["verdict"], mirror["verdict"]])
    assert ro["fixed"][1027] == 1 and ro["lost"][1029] == 1 and ro["count"] == [2, 4, ro["count"][2], 4]   # (a damaged CRC word is in no mirror)
    rebuild([con, h], ro, outs)


def test_refusals_that_need_a_device(gpu_ctx, oracle, cons):
    import ms_compress_amd as m
    h = healthy_of(gpu_ctx, cons, "xpress")
    ctx, nb = gpu_ctx, int(h.first[-1])
    good = np.full(h.nbt, SKIPPED, dtype=np.uint32); good[:nb] = GOOD
    dv = [i32(good, h.dev)]
    outs = repair_outs(h.dev, h.n, nb)
    refused = lambda call: pytest.raises(m.MSCompError, call).value.status == m.MSCOMP_ARG_ERROR
    dedupers = {"dedup": m.BlockDeduper(ctx, B, 1, h.n, h.nbt), "diff": m.BlockDeduper.for_diff(ctx, B, h.n, nb),
                "match": m.BlockDeduper.for_match(ctx, B, 1, 2 * h.n, 2 * h.nbt, h.nbt), "repair": m.BlockDeduper.for_repair(ctx, B, 1, h.n, nb)}
    z = lambda k: d64([], h.dev, k)
    st = i32(np.zeros(h.n, dtype=np.uint32), h.dev)
    for kind in ("dedup", "diff", "match"):                       # the wrong kind, in all directions
        k = dedupers[kind].n_src
        assert refused(lambda: dedupers[kind].repair([h.view()] * k, dv * k, *outs.tensors())), kind
    rp = dedupers["repair"]
    assert refused(lambda: rp.dedup([h.view()], z(h.n), z(h.n), z(2 * h.n), z(4), st))
    assert refused(lambda: rp.diff(h.view(), h.view(), z(2 * h.n), z(h.n + 1), z(4 * nb), z(h.n + 1), z(4 * nb), z(h.n), z(4), st))
    assert refused(lambda: rp.match([h.view()], h.view(), z(h.n + 1), z(4 * nb), z(h.n + 1), z(4 * nb), z(3 * h.n), z(6), st))
    t = outs.tensors()                                             # (ext_first, ext, fixed, lost, count, status)
    for i in range(6):                                            # null arrays
        assert refused(lambda: rp.repair([h.view()], dv, *[None if k == i else x for k, x in enumerate(t)])), i
    assert refused(lambda: rp.repair([h.view()], [None], *t))
    assert outs.untouched()
    for d in dedupers.values():
        d.close()
    so = SalvageOuts(h.dev, h.n, h.nbt, 64)
    args = [h.d_packed, h.d_first, h.d_boff, h.d_len, so.d_out, z(h.n), z(h.n), so.d_olen, so.d_bad, so.d_verdict, so.d_count, so.d_st]
    for i in range(12):                                           # salvage: every required array
        assert refused(lambda: h.bk.salvage(*[None if k == i else x for k, x in enumerate(args)], packed_len=h.plen)), i
    ctx.stream.synchronize()
    got = so.pull()
    assert set(got["verdict"]) == {SENT32} and set(got["count"]) == {SENT} and set(got["status"]) == {ST_FILL}
    # n_res = 0 and n_blocks_new = 0, and the room rule, against the model
    mo, _ = check_repair([h], [good], n=0, room=0)
    assert mo["ext_first"] == [0] and mo["count"] == [0, 0, 0, 0]
    mo, _ = check_repair([h], [good], room=0)
    assert mo["status"] == [0 if L == 0 else P.ARG for L in h.lens] and mo["ext"] == []
    mo, _ = check_repair([h, h], [good, good], room=int(h.first[P.TEXT + 1]) - 1)
    assert mo["status"][P.TEXT] == P.ARG and mo["status"][P.MIXED] == 0 and mo["status"][P.LAST] == 0
    mo, _ = check_repair([h, h], [good, good], n=h.n + 2)          # resources the primary does not have
    assert mo["status"][h.n:] == [P.ARG, P.ARG]
    empty = m.BlockContainer(ctx, FMTS["xpress"], B, 0, 0)         # a container of no resources: nothing to report on
    empty.salvage(None, z(1), z(1), None, None, None, None, None, None, None, None, None, packed_len=0)
    empty.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_scratch_independence(gpu_ctx, oracle, fmt):
    """the container's and the deduper's scratch poisoned before every call: the answers are the model's"""
    import ms_compress_amd as m
    h = Container.make(gpu_ctx, FMTS[fmt], B, R.buffers(B))       # (a container of its own: the poison stays with it)
    con = damaged(h, P.r_everything(h, oracle))
    nb = int(h.first[-1])
    dd = m.BlockDeduper.for_repair(gpu_ctx, B, 2, h.n, nb)
    outs = repair_outs(h.dev, h.n, nb)
    rep = m.api.scratch_report(dd, 0)
    assert list(rep) == ["tab"] and rep["tab"][0] == 32 * h.n + 4 * nb + 64 * ((nb + 1023) // 1024) + 72 and rep["tab"][1] >= rep["tab"][0]
    for byte in POISONS:
        assert m.api.scratch_poison(h.bk, byte) >= 1
        mo, _, _ = check_salvage(oracle, h, con, what=("poison", byte))
        assert m.api.scratch_poison(h.bk, byte) >= 1
        mi, _, _ = check_salvage(oracle, h, h, only=mo["verdict"], what=("poison, masked", byte))
        assert m.api.scratch_poison(dd, byte) == 1
        ro, _ = check_repair([con, h], [mo["verdict"], mi["verdict"]], dd=dd, outs=outs)
        assert m.api.scratch_report(dd, byte)["tab"][2] == 0, ("slack bytes touched", byte)
    rebuild([con, h], ro, outs)
    dd.close()
    h.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_salvage_repair_and_splice_in_one_captured_graph(oracle, fmt):
    """salvage(primary), salvage(mirror, only), repair and splice_extents, all executed for the first time inside one capture of the ctx
    stream; the graph is replayed twice, with other damage uploaded in place before the second replay"""
    import torch
    import ms_compress_amd as m
    f = FMTS[fmt]
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        h = Container.make(ctx, f, B, R.buffers(B))
        mirror_bk = m.BlockContainer(ctx, f, B, h.n, h.total)
        cases = [(P.r_mendable(h, oracle), P.r_crc_word(h, oracle)), (P.r_primary(h, oracle), P.r_mirror1(h, oracle))]
        own = lambda e: damaged(h, dict(e, packed=e.get("packed", h.packed), crc=e.get("crc", h.crc), off=e.get("off", h.off)))   # (arrays of its own)
        slots = [own(e) for e in cases[0]]                        # rewritten in place below
        nb = int(h.first[-1])
        out_off, room = h.layout(h.lens)
        so = [SalvageOuts(h.dev, h.n, h.nbt, room) for _ in slots]
        d_ooff, d_caps = d64(out_off, h.dev), d64(h.lens, h.dev)
        dd, sp = m.BlockDeduper.for_repair(ctx, B, 2, h.n, nb), m.BlockSplicer.for_extents(ctx, B, 2, h.n, nb, h.nbt)
        outs, built = repair_outs(h.dev, h.n, nb), Spliced(h.dev, h.n, h.nbt, 2 * h.plen + 32, True)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for k, (con, bk) in enumerate(zip(slots, (h.bk, mirror_bk))):
            bk.salvage(con.d_packed, con.d_first, con.d_boff, con.d_len, so[k].d_out, d_ooff, d_caps, so[k].d_olen, so[k].d_bad, so[k].d_verdict, so[k].d_count,
                       so[k].d_st, d_block_crc=con.d_crc, d_only=so[0].d_verdict if k else None, packed_len=con.cap)
        dd.repair([c.view() for c in slots], [x.d_verdict for x in so], *outs.tensors())
        built.run(sp, [c.view() for c in slots], outs["ext_first"], outs["ext"])
    for k, edits in enumerate(cases):
        held = [own(e) for e in edits]
        with torch.cuda.stream(s):
            for slot, con in zip(slots, held):
                slot.d_packed.copy_(con.d_packed); slot.d_boff.copy_(con.d_boff); slot.d_crc.copy_(con.d_crc)
            for x in so:
                x.reset()
            outs.reset(); built.fill()
            g.replay()
        s.synchronize()
        mo = P.model_salvage(oracle, f, held[0].model(), B, h.total, h.lens)
        mi = P.model_salvage(oracle, f, held[1].model(), B, h.total, h.lens, only=mo["verdict"])
        so[0].against(mo, out_off, B, ("primary, replay", k))
        so[1].against(mi, out_off, B, ("mirror, replay", k))
        ro = P.model_repair([c.model() for c in held], [mo["verdict"], mi["verdict"]], B, h.n, nb)
        outs.against(ro, exact=("ext_first", "fixed", "lost", "count"), prefixes=("ext",))
        assert (sum(ro["lost"]) == 0) == (k == 0)
        mb = P.model_rebuild([c.model() for c in held], ro, B, n_ext=nb, cap=built.room)
        built.against(mb, "rebuilt, replay %d" % k)
        if k == 0:
            assert bytes(built.as_built()["packed"][: h.plen]) == h.packed
    del g
    for x in (dd, sp, mirror_bk, h):
        x.close()
    ctx.close()


def test_host_conveniences(gpu_ctx, oracle):
    import ms_compress_amd as m
    f = FMTS["xpress_huff"]
    bufs = [text(7, 3 * B + 17), b"", recipe("mixed", 8, 2, 5, B), text(9, 3000)]
    healthy = Container.via_host(gpu_ctx, f, B, bufs)
    s = P.types.SimpleNamespace(fmt=f, B=B, packed=healthy.packed, first=healthy.first, off=healthy.off, lens=healthy.lens, crc=healthy.crc)
    primary = (P._flips(s, oracle, [(0, 1, False), (2, 1, True), (3, 0, False)]),) + healthy.host()[1:]
    mirror = (P._flips(s, oracle, [(0, 2, False), (3, 0, True)]),) + healthy.host()[1:]
    res, ver, bad, st, counts = m.blocks_salvage(f, *primary[:4], B, ctx=gpu_ctx, block_crc=primary[4])
    assert list(ver) == [GOOD, DECODE, GOOD, GOOD, GOOD, CRC, GOOD, DECODE] and bad == [1, 0, 1, 1] and st == [P.DATA, 0, P.DATA, P.DATA]
    assert counts == [8, 3, 2 * B + 3000, 3] and res[1] == b"" and res[3] == bytes(3000)
    assert res[0] == bufs[0][:B] + bytes(B) + bufs[0][2 * B:] and res[2] == bufs[2][:B] + bytes(B) + bufs[2][2 * B:]
    res, ver2, bad, st, counts = m.blocks_salvage(f, *mirror[:4], B, ctx=gpu_ctx, block_crc=mirror[4], only=ver)
    assert list(ver2) == [SKIPPED, GOOD, SKIPPED, SKIPPED, SKIPPED, GOOD, SKIPPED, CRC] and counts == [3, 1, 3000, 1]
    (packed, first, off, lens, crc), report = m.blocks_repair(f, [primary, mirror], B, ctx=gpu_ctx)
    assert report["fixed"] == [1, 0, 1, 0] and report["lost"] == [0, 0, 0, 1] and report["statuses"] == [0, 0, 0, P.DATA] and report["counts"][:2] == [2, 1]
    assert report["resources"][0] == [(0, 0, 0, 1), (1, 0, 1, 1), (0, 0, 2, 2)] and [list(v) for v in report["verdicts"]] == [list(ver), list(ver2)]
    assert lens == healthy.lens and np.array_equal(first, healthy.first) and np.array_equal(off, healthy.off) and np.array_equal(crc, healthy.crc)
    nb3 = int(healthy.off[P.row(s, 3)])
    assert bytes(packed[:nb3]) == healthy.packed[:nb3] and bytes(packed[nb3:]) == primary[0][nb3:], "the lost row is the primary's"
    out, st = m.blocks_decompress(f, packed, first, off, lens, B, ctx=gpu_ctx, block_crc=crc)
    assert st == [0, 0, 0, P.DATA] and out[:3] == bufs[:3]
