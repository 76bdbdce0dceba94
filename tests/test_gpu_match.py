"""GPU: mscomp_amd_deduper_match against the model of tests/match_model.py -- every entry of the seven outputs compared with sentinel-filled
arrays that are longer than the call may write (so a write behind the extents in use, or behind the last resource, fails) --, then the two
splices the header's consequence speaks of run on the GPU from the call's own device arrays: the delta lists over {new}, the patch lists
over {stores..., delta}; the rebuilt container is held to the extents model and, wherever every resource of new is accepted, byte for byte
to the new container. The containers are made by the GPU's blocks_compress / blocks_crc; the helpers are those of tests/blocks_rig.py."""
import numpy as np
import pytest

import blocks_model as M
import dedup_model as D
import diff_model as F
import match_model as T
import read_model as R
from blocks_rig import Container, ListOuts, Spliced, d64, memo, rand, recipe, same_lists, soft, table_only, FMTS, POISONS, SENT

pytestmark = pytest.mark.gpu
FOUND, SHARED, FRESH = T.FOUND, T.SHARED, T.FRESH
SHAPES = (("lznt1", 4096), ("xpress", 4096), ("xpress_huff", 4096), ("xpress", 65536))
TILE = 1024


EXACT, PREFIXES = ("delta_first", "patch_first", "cls", "count"), ("delta_ext", "patch_ext")


def Side(con, crc=True, nbt=None, plen=None):
    """a container as one view of a call states it: with or without its checksums, with other table rows or another packed length"""
    return con.edited(with_crc=crc, nbt=nbt, plen=plen)


def Outs(dev, n_new, n_all, room):
    """the seven output arrays of a match of n_new resources of new among n_all, within `room` new blocks, sentinel-filled and guarded"""
    outs = ListOuts(dev, {"delta_first": n_new + 1, "delta_ext": 4 * room, "patch_first": n_new + 1, "patch_ext": 4 * room, "cls": 3 * n_new, "count": 6}, n_all)
    outs.room = room
    return outs


def against_model(got, mo):
    ListOuts.compare(got, mo, exact=EXACT, prefixes=PREFIXES)


def check_match(stores, new, total=None, room=None, dd=None, outs=None):
    """one call compared with the model, array for array; returns (model, Outs)"""
    import ms_compress_amd as m
    ctx, B, dev = new.ctx, new.B, new.dev
    room = new.nbt if room is None else room
    total = sum(s.nbt for s in stores) + max(room, new.nbt) if total is None else total
    n_all = sum(s.n for s in stores) + new.n
    deduper = dd or m.BlockDeduper.for_match(ctx, B, len(stores), n_all, total, room)
    outs = outs or Outs(dev, new.n, n_all, room)
    outs.reset()
    deduper.match([s.view() for s in stores], new.view(), *outs.tensors())
    ctx.stream.synchronize()
    if dd is None:
        deduper.close()
    mo = T.model_match([s.model() for s in stores], new.model(), B, total, room, True)
    against_model(outs.pull(), mo)
    return mo, outs


def rebuild(stores, new, mo, outs, same=None):
    """the header's consequence on the GPU, from the device arrays the match left: the delta container out of {new}, then stores + delta"""
    import ms_compress_amd as m
    stores = list(stores)
    ctx, B, n, room = new.ctx, new.B, new.n, outs.room
    with_crc = all(s.with_crc for s in stores + [new])
    models = [s.model() for s in stores]
    md, mb = T.model_delta_and_patch(models, new.model(), mo, B, room, with_crc)
    delta = Spliced(new.dev, n, room, len(md["packed"]) + 32, with_crc)
    built = Spliced(new.dev, n, room, len(mb["packed"]) + 32, with_crc)
    cut = lambda s: s.view(crc=with_crc)
    s1, s2 = m.BlockSplicer.for_extents(ctx, B, 1, n, room, room), m.BlockSplicer.for_extents(ctx, B, len(stores) + 1, n, room, room)
    delta.run(s1, [cut(new)], outs["delta_first"], outs["delta_ext"])
    built.run(s2, [cut(s) for s in stores] + [delta.view()], outs["patch_first"], outs["patch_ext"])
    ctx.stream.synchronize()
    s1.close(); s2.close()
    delta.against(md, "delta")
    built.against(mb, "rebuilt")
    assert len(md["packed"]) == mo["count"][4] and int(md["first"][n]) == mo["count"][2]
    T.holds_consequence(models, new.model(), mo, B, room, with_crc)
    same = all(s == 0 for s in mo["status"][mo["n_store"]:]) if same is None else same
    if same:
        got = built.as_built()
        got["packed"] = got["packed"][: new.plen]
        F.same_container(got, new.model(with_crc, plen=new.plen)[:1] + (new.plen,) + new.model(with_crc)[2:], with_crc)
        assert int(got["off"][int(got["first"][new.n])]) == new.plen
    return md, mb


@pytest.fixture(scope="module")
def cons(gpu_ctx):
    """containers by name, made once"""
    yield from memo()


def raw_con(ctx, bufs, B=4096, f=3, crc=None):
    """random buffers as a container: every block is stored raw, the stored bytes are the data"""
    con = Container.via_host(ctx, f, B, bufs)
    assert bytes(con.packed) == b"".join(bufs)
    return con if crc is None else con.edited(crc=np.full(con.nbt, crc, dtype=np.uint32))


@pytest.mark.parametrize("fmt,B", SHAPES)
def test_identity_and_moves(gpu_ctx, cons, fmt, B):
    """resources of 0, 1, B - 1, B, B + 1, 3 B + 17 and 5 B bytes, raw and compressed blocks side by side"""
    bufs = R.buffers(B)
    store = cons((fmt, B, "recipes"), lambda: Container.via_host(gpu_ctx, FMTS[fmt], B, bufs))
    rows = sum(store.blocks(r) for r in range(store.n))
    for crc in (True, False):
        mo, outs = check_match([Side(store, crc)], Side(store, crc))              # identity: all found, D has no rows
        assert mo["count"][:5] == [rows, 0, 0, rows, 0] and mo["delta_ext"] == [] and mo["status"] == [0] * (2 * store.n)
        rebuild([Side(store, crc)], Side(store, crc), mo, outs)
    moved = [bufs[k] for k in (9, 0, 5, 3, 11, 1)] + [rand(31, B) + bufs[7], bufs[8][: 2 * B] + bufs[4], bufs[7][2 * B: 3 * B] + bufs[2]]
    new = cons((fmt, B, "moved"), lambda: Container.via_host(gpu_ctx, FMTS[fmt], B, moved))
    for crc in (True, False):
        mo, outs = check_match([Side(store, crc)], Side(new, crc))
        assert mo["count"][1:3] == [0, 1] and mo["count"][5] == 0
        assert mo["patch_ext"][mo["patch_first"][6]: mo["patch_first"][7]] == [(1, 6, 0, 1), (0, 7, 0, 4)]     # one block inserted at the front: ONE run behind it
        assert mo["patch_ext"][mo["patch_first"][7]:] == [(0, 8, 0, 2), (0, 4, 0, 2), (0, 7, 2, 1), (0, 2, 0, 1)]   # a concatenation; a block moved to another resource
        rebuild([Side(store, crc)], Side(new, crc), mo, outs)
    mo, outs = check_match([Side(store, True)], Side(new, False))                   # a null d_block_crc in one view: no checksum takes part
    assert mo["count"][2] == 1
    mo, outs = check_match([], new)                                                 # no store: the blocks that stand twice in the container are shared
    rebuild([], new, mo, outs)


def test_sharing(gpu_ctx):
    B = 4096
    x, y, z = rand(5, B), rand(6, B), rand(7, B)
    new = raw_con(gpu_ctx, [x + y + x, z + x, x + y, y + x])
    mo, outs = check_match([], new)
    assert mo["classes"] == [[FRESH, FRESH, SHARED], [FRESH, SHARED], [SHARED, SHARED], [SHARED, SHARED]]
    assert mo["patch_ext"][4:] == [(0, 0, 0, 2), (0, 0, 1, 1), (0, 0, 0, 1)]        # representatives consecutive: one run; swapped: two
    assert mo["count"] == [0, 6, 3, 9, 3 * B, 0]
    rebuild([], new, mo, outs)
    thrice = raw_con(gpu_ctx, [x + x, rand(8, B) + x])                               # the same fresh block three times, within one resource and across two
    mo, outs = check_match([raw_con(gpu_ctx, [y])], thrice)
    assert mo["classes"] == [[FRESH, SHARED], [FRESH, SHARED]] and mo["patch_ext"] == [(1, 0, 0, 1), (1, 0, 0, 1), (1, 1, 0, 1), (1, 0, 0, 1)]
    rebuild([raw_con(gpu_ctx, [y])], thrice, mo, outs)
    zeros = Container.via_host(gpu_ctx, 2, B, [bytes(5 * B)])                                  # the smallest equal row always wins: one extent per block
    mo, outs = check_match([], zeros)
    assert mo["patch_ext"] == [(0, 0, 0, 1)] * 5 and mo["count"][:3] == [0, 4, 1]
    rebuild([], zeros, mo, outs)


def test_smallest_wins_and_short_blocks(gpu_ctx):
    B = 4096
    x, t = rand(8, B), rand(9, 100)
    s0, s1 = raw_con(gpu_ctx, [rand(10, B), x + t]), raw_con(gpu_ctx, [x, x + t, x[:100]])
    new = raw_con(gpu_ctx, [x + t, t, x[:100], x[:50]])
    mo, outs = check_match([s0, s1], new)
    assert mo["patch_ext"] == [(0, 1, 0, 2), (0, 1, 1, 1), (1, 2, 0, 1), (2, 3, 0, 1)] and mo["count"][:3] == [4, 0, 1]
    rebuild([s0, s1], new, mo, outs)
    mo, outs = check_match([s1, s0], new)                                           # the other order: twice in one store, the smaller row wins
    assert mo["patch_ext"][:3] == [(0, 0, 0, 1), (0, 1, 1, 1), (0, 1, 1, 1)]
    rebuild([s1, s0], new, mo, outs)
    twice = raw_con(gpu_ctx, [t, t, x + t])                                         # equal tails are shared too
    mo, outs = check_match([], twice)
    assert mo["classes"] == [[FRESH], [SHARED], [FRESH, SHARED]]
    rebuild([], twice, mo, outs)
    a, other = raw_con(gpu_ctx, [x + t]), raw_con(gpu_ctx, [t])
    mo, outs = check_match([a], other)
    assert mo["count"][:3] == [1, 0, 0]
    for crc in (True, False):
        fat = Side(other.edited(lens=[200]), crc)                                   # the same stored bytes and CRC word, another data length: that clause decides
        mo, outs = check_match([Side(a, crc)], fat)
        assert mo["count"][:3] == [0, 0, 1] and mo["status"] == [0, 0]
        thin = Side(a.edited(lens=[B + 200]), crc)                                  # and the other way round
        mo, outs = check_match([thin], Side(other, crc))
        assert mo["count"][:3] == [0, 0, 1]


@pytest.mark.parametrize("crc", (None, 0x1234))
def test_refuted_chain(gpu_ctx, crc):
    """raw blocks that agree in length and in their first and last 16 bytes and differ in the middle: x1 < x2 in the store; x2, x3, x3 in new.
    Without checksums, and with checksums whose words are edited on the host to agree"""
    B = 4096
    x1, x2, x3 = D.same_ends([rand(21, B), rand(22, B), rand(23, B)], B)
    store, new = raw_con(gpu_ctx, [x1 + x2], crc=crc), raw_con(gpu_ctx, [x2 + x3 + x3], crc=crc)
    sides = ([Side(store, crc is not None)], Side(new, crc is not None))
    mo, outs = check_match(*sides)
    assert mo["patch_ext"] == [(0, 0, 1, 1), (1, 0, 0, 1), (1, 0, 0, 1)]             # x2 at x2's row, not x1's; x3 fresh, then shared
    assert mo["classes"] == [[FOUND, FRESH, SHARED]] and mo["count"] == [1, 1, 1, 3, B, 4]
    rebuild(*sides, mo, outs)
    mo, outs = check_match([], sides[1])                                             # the chain inside one container
    assert mo["classes"] == [[FRESH, FRESH, SHARED]] and mo["count"][5] == 2
    rebuild([], sides[1], mo, outs)


def test_damaged_tables(gpu_ctx, cons):
    B, fmt = 4096, "xpress"
    bufs = [rand(41, 2 * B), rand(42, 3 * B + 17), rand(43, B), b"", soft(44, B + 1)]
    good = cons((fmt, B, "damage"), lambda: Container.via_host(gpu_ctx, FMTS[fmt], B, bufs))
    n, lens = good.n, good.lens
    falling = good.first.copy(); falling[1] = falling[2] + np.uint64(1)               # resource 1 by rule 1; resource 0 gets rows too many: rule 2
    odd = list(lens); odd[1] += B                                                    # rule 2
    j = int(good.first[1])
    back = good.off.copy(); back[j + 2] = back[j + 1] - np.uint64(1)                 # rule 3: a decreasing entry inside resource 1
    last = int(good.off[int(good.first[4])])
    hurt = {"falling": (Side(good.edited(first=falling)), {1: M.ARG, 0: M.DATA}), "odd": (Side(good.edited(lens=odd)), {1: M.DATA}),
            "back": (Side(good.edited(off=back)), {1: M.DATA}),
            "short": (Side(good, plen=last + 1), {4: M.DATA})}                      # rule 3: the stored bytes of resource 4 lie beyond a short packed_len
    blocks = [good.blocks(r) for r in range(n)]
    for name, (con, bad) in hurt.items():
        mo, outs = check_match([con], good)                                          # a refused store resource brings no rows: its blocks are fresh
        assert mo["status"] == [bad.get(r, 0) for r in range(n)] + [0] * n, name
        assert mo["cls"] == [x for r in range(n) for x in ((0, 0, blocks[r]) if r in bad else (blocks[r], 0, 0))], name
        rebuild([con], good, mo, outs)
        mo, outs = check_match([good], con)                                          # a refused resource of new: no extents, zero counts; indices never shift
        assert mo["status"] == [0] * n + [bad.get(r, 0) for r in range(n)], name
        assert [e[1] for e in mo["patch_ext"]] == [r for r in range(n) if lens[r] and r not in bad] and mo["count"][1:3] == [0, 0], name
        rebuild([good], con, mo, outs)
    # rule 4. Resources 0 and 2 of `twice` both claim rows 0 and 1 of a table of two rows, resource 1 falls by rule 1 between them
    x = rand(45, 2 * B)
    one = raw_con(gpu_ctx, [x, b"", x])
    twice = Side(one.edited(first=np.array([0, 2, 0, 2], dtype=np.uint64)), nbt=2, plen=2 * B)
    store = Side(raw_con(gpu_ctx, [rand(46, B)]), nbt=1)                             # one row
    for total, room, want in ((5, 4, 0), (5, 3, M.ARG), (4, 4, M.ARG), (3, 2, M.ARG)):
        mo, outs = check_match([store], twice, total=total, room=room)               # at exactly the bound, and one beyond it
        assert mo["status"] == [0, 0, M.ARG, want] and mo["classes"][2] == (None if want else [SHARED, SHARED]), (total, room)
        rebuild([store], twice, mo, outs, same=False)
    mo, outs = check_match([twice], store, total=3, room=1)                         # refused in a store: it has counted, new's resource falls too
    assert mo["status"] == [0, M.ARG, M.ARG, M.ARG] and mo["count"][:4] == [0, 0, 0, 0]


def test_tiles(gpu_ctx):
    """one resource of 2 TILE + 3 blocks: a found run across both tile boundaries; a class change exactly on a boundary; a shared run whose
    representatives lie in another tile"""
    B, f = 4096, FMTS["lznt1"]
    rows = 2 * TILE + 3
    s, fr = soft(1, rows * B), soft(2, 10 * B)
    store = Container.via_host(gpu_ctx, f, B, [s])
    wide = Container.via_host(gpu_ctx, f, B, [fr[:B] + s[: (rows - 1) * B]])
    mo, outs = check_match([store], wide)
    assert mo["patch_ext"] == [(1, 0, 0, 1), (0, 0, 0, rows - 1)] and mo["delta_ext"] == [(0, 0, 0, 1)]
    rebuild([store], wide, mo, outs)
    tail = rows - (TILE + 6)
    data = fr + s[10 * B: TILE * B] + fr[2 * B: 8 * B] + s[100 * B: (100 + tail) * B]
    edge = Container.via_host(gpu_ctx, f, B, [data])
    assert edge.blocks(0) == rows
    mo, outs = check_match([store], edge)
    assert mo["patch_ext"] == [(1, 0, 0, 10), (0, 0, 10, TILE - 10), (1, 0, 2, 6), (0, 0, 100, tail)] and mo["count"][:3] == [rows - 16, 6, 10]
    rebuild([store], edge, mo, outs)
    mo, outs = check_match([], edge)                                                # no store: a shared run of 924 rows whose representatives lie a tile back
    assert mo["patch_ext"] == [(0, 0, 0, TILE), (0, 0, 2, 6), (0, 0, 100, TILE - 100), (0, 0, TILE, tail - (TILE - 100))]
    rebuild([], edge, mo, outs)


def test_tile_scan_second_trip(gpu_ctx):
    """1024 * 1024 + 3 rows of next, hand-made tables and no stored byte, no store: the one-workgroup scan over the tiles' words takes a
    second trip of 1024 tiles. Every row has the stored length 0, so all share one key: row 0 is fresh, and every later row is a shared
    run of one row whose representative is row 0 -- a patch extent per row, its place in the list the running sum carried over the
    trips. The expectations are closed forms; the same construction at 2 * 1024 + 3 rows is held to the model first, which is what
    they rest on."""
    import ms_compress_amd as m
    B = 4096

    def case(rows):
        want = {"delta_first": [0, 1], "delta_ext": [0, 0, 0, 1], "patch_first": [0, rows], "patch_ext": np.tile(np.array([0, 0, 0, 1], dtype=np.uint64), rows),
                "cls": [0, rows - 1, 1], "count": [0, rows - 1, 1, rows, 0, 0], "status": [0]}
        return table_only(gpu_ctx, B, [rows]), want

    con, want = case(2 * TILE + 3)
    _, outs = check_match([], con)
    same_lists(outs, want)
    rows = TILE * TILE + 3
    con, want = case(rows)
    dd, outs = m.BlockDeduper.for_match(gpu_ctx, B, 0, 1, rows, rows), Outs(con.dev, 1, 1, rows)
    dd.match([], con.view(), *outs.tensors())
    gpu_ctx.stream.synchronize()
    dd.close()
    same_lists(outs, want)


def test_degenerate(gpu_ctx, cons):
    import torch
    import ms_compress_amd as m
    B = 4096
    some = raw_con(gpu_ctx, [rand(61, B + 5), rand(62, 3 * B)])
    none = Container.from_host(gpu_ctx, 3, B, b"", [0], [0], [], [])
    mo, outs = check_match([some], none)                                            # an empty new container
    assert mo["count"] == [0] * 6 and mo["delta_first"] == [0] and mo["patch_first"] == [0]
    mo, outs = check_match([none, none, none], some)                                # stores without a resource
    assert mo["count"][:4] == [0, 0, 5, 5]
    rebuild([none, none, none], some, mo, outs)
    mo, outs = check_match([some], Side(some, nbt=0), room=0)                       # n_blocks_new = 0: every resource with blocks falls by rule 1
    assert mo["status"] == [0, 0, M.ARG, M.ARG] and mo["count"] == [0] * 6
    dead = Side(some.edited(lens=[1, 2]))                                           # a store with no accepted resource
    mo, outs = check_match([dead], some)
    assert mo["status"] == [M.DATA, M.DATA, 0, 0] and mo["count"][:3] == [0, 0, 5]
    rebuild([dead], some, mo, outs)
    d0 = m.BlockDeduper.for_match(gpu_ctx, B, 0, 0, 0, 0)                           # nothing at all: d_count alone is required
    cnt = torch.full((6,), SENT, dtype=torch.int64, device=some.dev)
    d0.match([], none.view(), None, None, None, None, None, cnt, None)
    gpu_ctx.stream.synchronize()
    assert cnt.cpu().tolist() == [0] * 6
    d0.close()


def busy_case(gpu_ctx, cons, fmt, B=4096):
    """two stores and a new container with every class in it, runs of every kind, a refuted chain, a refused store resource and a refused
    resource of new between accepted ones"""
    bufs = R.buffers(B)
    x1 = rand(21, B)
    x2, x3 = D.crc_twin(x1, 1000), D.crc_twin(x1, 2000)                             # equal CRC words, equal ends, other bytes: one key tuple
    s0 = cons((fmt, B, "busy0"), lambda: Container.via_host(gpu_ctx, FMTS[fmt], B, [bufs[5], bufs[7], x1 + x2]))
    s1 = cons((fmt, B, "busy1"), lambda: Container.via_host(gpu_ctx, FMTS[fmt], B, [bufs[9], bufs[4], bufs[8]]))
    new = cons((fmt, B, "busy2"), lambda: Container.via_host(gpu_ctx, FMTS[fmt], B, [rand(71, B) + bufs[7], bufs[9][B: 3 * B] + rand(72, 2 * B) + bufs[4], x2 + x3 + x3,
                                                                          b"", bufs[8], rand(72, 2 * B)]))
    odd = list(s1.lens); odd[2] += B
    cut = list(new.lens); cut[3] = 1
    return [Side(s0), Side(s1.edited(lens=odd))], Side(new.edited(lens=cut))


@pytest.mark.parametrize("fmt", list(FMTS))
def test_five_executions_are_identical(gpu_ctx, cons, fmt):
    """the first execution launches, the later ones replay the object's graph; a changed field of a view captures again"""
    import ms_compress_amd as m
    stores, new = busy_case(gpu_ctx, cons, fmt)
    room, total, n_all = new.nbt + 3, stores[0].nbt + stores[1].nbt + new.nbt + 5, stores[0].n + stores[1].n + new.n + 2
    dd = m.BlockDeduper.for_match(gpu_ctx, new.B, 2, n_all, total, room)
    outs = Outs(new.dev, new.n, n_all - 2, room)
    seen = []
    for _ in range(5):
        mo, _ = check_match(stores, new, total=total, room=room, dd=dd, outs=outs)
        seen.append(outs.pull())
    assert mo["count"][5] == 4 and mo["status"] == [0, 0, 0, 0, 0, M.DATA, 0, 0, 0, M.DATA, 0, 0]
    assert mo["count"][0] == 9 and mo["count"][1] == 3 and mo["count"][2] == 4 + 4           # bufs[8] fell with its store resource: its four blocks are fresh
    assert all(s == seen[0] for s in seen)
    rebuild(stores, new, mo, outs)
    short = Side(new, plen=new.cap - 1)                                        # one field of one view changed: captured again, and answered for what it says
    mo2, _ = check_match(stores, short, total=total, room=room, dd=dd, outs=outs)
    assert mo2["status"][-1] == M.DATA and mo2["status"][:-1] == mo["status"][:-1]
    mo3, _ = check_match(stores, new, total=total, room=room, dd=dd, outs=outs)
    assert outs.pull() == seen[0]
    dd.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_scratch_contract(gpu_ctx, cons, fmt):
    """the scheme of tests/test_gpu_scratch.py: what an execution reads from the scratch it has written itself, and no pass touches the slack"""
    import ms_compress_amd as m
    stores, new = busy_case(gpu_ctx, cons, fmt)
    room, total, n_all = new.nbt + 3, stores[0].nbt + stores[1].nbt + new.nbt + 5, stores[0].n + stores[1].n + new.n
    dd = m.BlockDeduper.for_match(gpu_ctx, new.B, 2, n_all, total, room)
    outs = Outs(new.dev, new.n, n_all, room)
    check_match(stores, new, total=total, room=room, dd=dd, outs=outs)
    first = outs.pull()
    rep = m.api.scratch_report(dd, 0)
    assert list(rep) == ["tab"] and rep["tab"][0] == 48 * n_all + 40 * total + 4 * room + 64 * ((room + 1023) // 1024) + 848 and rep["tab"][1] >= rep["tab"][0]
    for byte in POISONS:
        assert m.api.scratch_poison(dd, byte) == 1                                   # the whole buffer, under the deduper's kind
        check_match(stores, new, total=total, room=room, dd=dd, outs=outs)
        assert outs.pull() == first, "after poison 0x%02X" % byte
        rep = m.api.scratch_report(dd, byte)
        assert rep["tab"][2] == 0, ("slack bytes touched", byte, rep)
    dd.close()


def test_wrong_kinds_and_nulls(gpu_ctx, cons):
    """each of the three kinds of deduper refuses the other two calls; every array missing in turn; views beyond the creation bounds"""
    import torch
    import ms_compress_amd as m
    B = 4096
    good = raw_con(gpu_ctx, [rand(81, 2 * B + 1), rand(82, B)])
    n, dev, v = good.n, good.dev, good.view()
    outs = Outs(dev, n, 2 * n, good.nbt)
    full = outs.tensors()
    pair = d64([0, 0, 1, 1], dev)
    spare = lambda k: torch.full((k,), SENT, dtype=torch.int64, device=dev)
    kinds = {"dedup": m.BlockDeduper(gpu_ctx, B, 2, 2 * n, 2 * good.nbt), "diff": m.BlockDeduper.for_diff(gpu_ctx, B, n, good.nbt),
             "match": m.BlockDeduper.for_match(gpu_ctx, B, 1, 2 * n, 2 * good.nbt, good.nbt)}
    calls = {"dedup": lambda dd: dd.dedup([v] * dd.n_src, spare(2 * n), spare(2 * n), spare(4 * n), outs["count"], outs.status),
             "diff": lambda dd: dd.diff(v, v, pair, outs["delta_first"], outs["delta_ext"], outs["patch_first"], outs["patch_ext"], spare(n), outs["count"], outs.status),
             "match": lambda dd: dd.match([v] * dd.n_src, v, *full)}
    for made, dd in kinds.items():
        for call, run in calls.items():
            if call != made:
                with pytest.raises(m.MSCompError) as e:
                    run(dd)
                assert e.value.status == m.MSCOMP_ARG_ERROR, (made, call)
    dm = kinds["match"]
    for k in range(len(full)):                                     # every array missing in turn
        with pytest.raises(m.MSCompError) as e:
            dm.match([v], v, *(full[:k] + (None,) + full[k + 1:]))
        assert e.value.status == m.MSCOMP_ARG_ERROR, k
    for broken in (v[:1] + (None,) + v[2:], v[:2] + (None,) + v[3:], v[:3] + (None,) + v[4:], (None,) + v[1:]):   # a view without a table, or without stored bytes
        for a, b in ((broken, v), (v, broken)):
            with pytest.raises(m.MSCompError) as e:
                dm.match([a], b, *full)
            assert e.value.status == m.MSCOMP_ARG_ERROR
    import ctypes as C
    views = m.api._blocks_views([v, v])
    ptrs = [C.c_void_p(t.data_ptr()) for t in full]
    assert gpu_ctx.lib.mscomp_amd_deduper_match(dm._h, None, C.byref(views[1]), *ptrs) == m.MSCOMP_ARG_ERROR      # a null store array with n_src = 1
    assert gpu_ctx.lib.mscomp_amd_deduper_match(dm._h, views, None, *ptrs) == m.MSCOMP_ARG_ERROR
    # the views' totals beyond the creation bounds: refused on the host, nothing launched
    for tight in (m.BlockDeduper.for_match(gpu_ctx, B, 1, 2 * n - 1, 2 * good.nbt, good.nbt), m.BlockDeduper.for_match(gpu_ctx, B, 1, 2 * n, 2 * good.nbt - 1, good.nbt),
                  m.BlockDeduper.for_match(gpu_ctx, B, 1, 2 * n, 2 * good.nbt, good.nbt - 1)):
        with pytest.raises(m.MSCompError) as e:
            tight.match([v], v, *full)
        assert e.value.status == m.MSCOMP_ARG_ERROR
        tight.close()
    torch.cuda.synchronize()
    assert outs.untouched()
    for dd in kinds.values():
        dd.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_match_and_both_splices_in_one_captured_graph(fmt):
    """match, the delta splice and the patch splice, all executed for the first time inside one capture of the ctx stream; the graph is then
    replayed on the containers it was captured with and on a second set of the same bounds, loaded into the same device arrays"""
    import torch
    import ms_compress_amd as m
    f, B = FMTS[fmt], 4096
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        a = [recipe("text", 4, 6, 33, B), recipe("random", 5, 2, 0, B)]
        b = [recipe("mixed", 31, 6, 33, B), recipe("text", 33, 2, 0, B)]
        fresh = rand(91, B)
        shape = lambda src: [src[1] + src[0][: 2 * B], fresh + src[0][2 * B: 4 * B] + fresh]     # the same lengths for either set
        sets = [(Container.via_host(ctx, f, B, src), Container.via_host(ctx, f, B, shape(src))) for src in (a, b)]
        assert sets[0][0].lens == sets[1][0].lens and sets[0][1].lens == sets[1][1].lens
        cap = max(c.plen for pair in sets for c in pair) + 100
        slots = [Container.from_host(ctx, f, B, c.packed, c.first, c.off, c.lens, c.crc, cap=cap) for c in sets[0]]
        n, room, n_all = slots[1].n, slots[1].nbt, slots[0].n + slots[1].n
        outs = Outs(slots[1].dev, n, n_all, room)
        dd = m.BlockDeduper.for_match(ctx, B, 1, n_all, slots[0].nbt + room, room)
        s1, s2 = m.BlockSplicer.for_extents(ctx, B, 1, n, room, room), m.BlockSplicer.for_extents(ctx, B, 2, n, room, room)
        delta, built = Spliced(slots[1].dev, n, room, cap, True), Spliced(slots[1].dev, n, room, cap, True)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        dd.match([slots[0].view()], slots[1].view(), *outs.tensors())
        delta.run(s1, [slots[1].view()], outs["delta_first"], outs["delta_ext"])
        built.run(s2, [slots[0].view(), delta.view()], outs["patch_first"], outs["patch_ext"])
    for k, (store, new) in enumerate((sets[0], sets[1], sets[0])):
        with torch.cuda.stream(s):
            for slot, con in zip(slots, (store, new)):
                slot.d_packed.fill_(0x3C); slot.d_packed[: con.plen] = con.d_packed[: con.plen]
                slot.d_first.copy_(con.d_first); slot.d_boff.copy_(con.d_boff); slot.d_crc.copy_(con.d_crc)
            outs.reset(); delta.fill(); built.fill()
            g.replay()
        s.synchronize()
        held = [Container.from_host(ctx, f, B, c.packed + b"\x3C" * (cap - c.plen), c.first, c.off, c.lens, c.crc).model() for c in (store, new)]   # what the slots hold
        mo = T.model_match(held[:1], held[1], B, slots[0].nbt + room, room, True)
        against_model(outs.pull(), mo)
        assert mo["count"][:3] == [new.blocks(0) + 2, 1, 1], k
        md, mb = T.model_delta_and_patch(held[:1], held[1], mo, B, room, True)
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
    extra = recipe("text", 44, 1, 0, B)
    new = [old[3], extra + old[0], b"", old[1] + old[0][: 2 * B], extra]
    made = []
    for bufs in (old, new):
        packed, first, off, st = m.blocks_compress(f, bufs, B, ctx=gpu_ctx)
        bcrc, _ = m.blocks_crc(f, bufs, B, ctx=gpu_ctx)
        made.append((packed, first, off, [len(b) for b in bufs], bcrc))
    delta_res, patch_res, classes, counts, st = m.blocks_match([made[0]], made[1], B, ctx=gpu_ctx)
    assert st == [0] * 9 and classes == [(2, 0, 0), (4, 0, 1), (0, 0, 0), (4, 0, 0), (0, 1, 0)] and counts[:4] == [10, 1, 1, 12] and counts[5] == 0
    assert delta_res == [[], [(0, 1, 0, 1)], [], [], []]
    assert patch_res == [[(0, 3, 0, 2)], [(1, 1, 0, 1), (0, 0, 0, 4)], [], [(0, 1, 0, 2), (0, 0, 0, 2)], [(1, 1, 0, 1)]]
    delta, patch2, classes2, counts2, st2 = m.blocks_match_delta([made[0]], made[1], B, ctx=gpu_ctx)
    assert (patch2, classes2, counts2, st2) == (patch_res, classes, counts, st)
    assert len(delta[0]) == counts[4] < len(made[1][0]) and [int(x) for x in delta[1]] == [0, 0, 1, 1, 1, 1]
    packed, first, off, lens, crc, status = m.blocks_match_patch([made[0]], delta, patch_res, B, ctx=gpu_ctx)
    assert status == [0] * 5 and lens == made[1][3]
    assert bytes(packed) == bytes(made[1][0]) and (first == made[1][1]).all() and (off == made[1][2]).all() and (crc == made[1][4]).all()
    out, dst = m.blocks_decompress(f, packed, first, off, lens, B, ctx=gpu_ctx, block_crc=crc)
    assert dst == [0] * 5 and out == new
    single, recipe_res, cls1, cnt1, st1 = m.blocks_single_instance(made[1], B, ctx=gpu_ctx)      # no store: the repeated blocks stored once
    assert st1 == [0] * 5 and cnt1[1] > 0 and len(single[0]) == cnt1[4] < len(made[1][0])
    packed, first, off, lens, crc, status = m.blocks_match_patch([], single, recipe_res, B, ctx=gpu_ctx)
    assert status == [0] * 5 and bytes(packed) == bytes(made[1][0]) and (off == made[1][2]).all() and (crc == made[1][4]).all()
