"""GPU: mscomp_amd_deduper_match_digest against the model of tests/match_digest_model.py -- every entry of the seven outputs compared with
sentinel-filled arrays that are longer than the call may write --, beside mscomp_amd_deduper_match where the header's consequence says the
two agree, and with the two splices run from the call's own device arrays. The containers are made by the GPU's blocks_compress /
blocks_crc, the columns by its BlockDigester (blocks_digest) or by hand; the helpers are those of tests/blocks_rig.py and, where match's
own tests have them already, of tests/test_gpu_match.py. B = 4096 throughout."""
import copy
import ctypes as C

import numpy as np
import pytest

import blocks_model as M
import digest_model as DM
import match_digest_model as G
import match_model as T
import read_model as R
import test_gpu_match as TM
from blocks_rig import Container, Spliced, d64, i32, memo, rand, recipe, soft, FMTS, POISONS, SENT

pytestmark = pytest.mark.gpu
FOUND, SHARED, FRESH = T.FOUND, T.SHARED, T.FRESH
B, TILE = 4096, 1024
Side, Outs, raw_con, rebuild = TM.Side, TM.Outs, TM.raw_con, TM.rebuild


def with_col(con, bufs=None, col=None):
    """a copy of ``con`` that brings its digest column: the BlockDigester's over ``bufs`` (held to the digest model), or the made-up rows
    ``col``; on the host as the model reads it (dig: nbt rows of four words) and on the device (d_dig, one spare row behind it)"""
    import ms_compress_amd as m
    c = copy.copy(con)
    if col is None:
        col = m.blocks_digest(bufs, con.B, ctx=con.ctx)
        assert (col == DM.store_digests(bufs, con.B, len(col))).all()
    h = np.zeros((con.nbt + 1, 4), dtype=np.uint32)
    col = np.asarray(col, dtype=np.uint32).reshape(-1, 4)
    h[: len(col)] = col
    c.dig, c.d_dig = h[: con.nbt].copy(), i32(h.reshape(-1), con.dev)
    return c


def recol(con, col):
    """``con`` with another column in a device tensor of its own"""
    return with_col(con, col=col)


def bare(view):
    """a source tuple without its payload: d_packed is null, the packed length stays"""
    return (None,) + tuple(view[1:])


def tab_con(ctx, lens, stored=7):
    """hand-made tables and no stored byte: resources of these lengths, every row of stored length ``stored``"""
    rows = [(L + B - 1) // B for L in lens]
    nbt = int(sum(rows))
    con = Container.from_host(ctx, FMTS["xpress"], B, b"", np.concatenate([[0], np.cumsum(rows)]), np.arange(nbt + 1, dtype=np.uint64) * np.uint64(stored),
                              lens, np.zeros(nbt, dtype=np.uint32))
    return con.edited(plen=stored * nbt)


def ids(*rows):
    """made-up digests: per row an id, or the four words themselves"""
    return np.array([r if isinstance(r, tuple) else (r, 3 * r + 1, 0xD16E57, r ^ 0x5A5A) for r in rows], dtype=np.uint32).reshape(-1, 4)


def check(stores, new, total=None, room=None, dd=None, outs=None, payload=True):
    """one call compared with the model, array for array; returns (model, Outs)"""
    import ms_compress_amd as m
    ctx, dev = new.ctx, new.dev
    room = new.nbt if room is None else room
    total = sum(s.nbt for s in stores) + max(room, new.nbt) if total is None else total
    n_all = sum(s.n for s in stores) + new.n
    matcher = dd or m.BlockDigestMatcher(ctx, B, len(stores), n_all, total, room)
    outs = outs or Outs(dev, new.n, n_all, room)
    outs.reset()
    cut = (lambda v: v) if payload else bare
    matcher.match([cut(s.view()) for s in stores], [s.d_dig for s in stores], cut(new.view()), new.d_dig, *outs.tensors())
    ctx.stream.synchronize()
    if dd is None:
        matcher.close()
    mo = G.model_match_digest([s.model() for s in stores], [s.dig for s in stores], new.model(), new.dig, B, total, room)
    TM.against_model(outs.pull(), mo)
    return mo, outs


@pytest.fixture(scope="module")
def cons(gpu_ctx):
    """containers by name, made once"""
    yield from memo()


def moved_bufs(bufs):
    return [bufs[k] for k in (9, 0, 5, 3, 11, 1)] + [rand(31, B) + bufs[7], bufs[8][: 2 * B] + bufs[4], bufs[7][2 * B: 3 * B] + bufs[2]]


def pair(gpu_ctx, cons, fmt, what):
    """the "recipes" or the "moved" container of tests/test_gpu_match.py in format fmt, with its true column"""
    bufs = R.buffers(B) if what == "recipes" else moved_bufs(R.buffers(B))
    return cons((fmt, what), lambda: with_col(Container.via_host(gpu_ctx, FMTS[fmt], B, bufs), bufs)), bufs


# ---- 1. agreement with match ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FMTS))
def test_agrees_with_match(gpu_ctx, cons, fmt):
    """resources of 0, 1, B - 1, B, B + 1, 3 B + 17 and 5 B bytes, healthy containers of one format with checksums and true columns: every
    output is match's, the refuted count apart, and both splices rebuild next byte for byte"""
    store, _ = pair(gpu_ctx, cons, fmt, "recipes")
    new, _ = pair(gpu_ctx, cons, fmt, "moved")
    for stores, nxt in (([store], store), ([store], new), ([], new), ([new, store], store)):
        mo, outs = check(stores, nxt)
        got = outs.pull()
        mm, mouts = TM.check_match(stores, nxt)
        want = mouts.pull()
        assert got["count"][:5] == want["count"][:5] and mo["count"][5] == 0
        assert all(got[k] == want[k] for k in got if k != "count")
        for k in ("status", "cls", "delta_first", "patch_first", "delta_ext", "patch_ext", "rep"):
            assert mo[k] == mm[k], k
        rebuild(stores, nxt, mo, outs)
    mo, _ = check([store], new)
    assert mo["count"][1:3] == [0, 1] and mo["patch_ext"][mo["patch_first"][6]: mo["patch_first"][7]] == [(1, 6, 0, 1), (0, 7, 0, 4)]


# ---- 2. across codecs -------------------------------------------------------------------------------------------------------------------
def test_across_codecs(gpu_ctx, cons):
    """an LZNT1 next against an Xpress and an Xpress+Huffman store in ONE call: the classes, the counts and the delta list of the one-format
    answer; the delta splices; the patch list, applied as a read recipe through ranged decodes, gives next's data"""
    import ms_compress_amd as m
    bufs = R.buffers(B)
    sb = [bufs[:6], bufs[6:]]
    nb = moved_bufs(bufs) + [bufs[9][B: 2 * B] + rand(32, 100), rand(33, B) + rand(33, B)]
    fm = ("xpress", "xpress_huff")
    stores = [cons(("x", f), lambda f=f, b=b: with_col(Container.via_host(gpu_ctx, FMTS[f], B, b), b)) for f, b in zip(fm, sb)]
    same = [cons(("x1", i), lambda b=b: with_col(Container.via_host(gpu_ctx, FMTS["lznt1"], B, b), b)) for i, b in enumerate(sb)]
    new = cons(("x", "new"), lambda: with_col(Container.via_host(gpu_ctx, FMTS["lznt1"], B, nb), nb))
    mo, outs = check(stores, new)
    one, _ = TM.check_match(same, new)                                             # the one-format answer, by stored bytes
    for k in ("status", "cls", "classes", "delta_first", "delta_ext", "patch_first", "patch_ext"):
        assert mo[k] == one[k], k
    assert mo["count"][:5] == one["count"][:5] and mo["count"][2] > 0 and mo["count"][0] > 0 and mo["count"][1] > 0
    fresh_bytes = sum(int(new.off[int(new.first[q]) + k + 1] - new.off[int(new.first[q]) + k]) for q in range(new.n)
                      for k, c in enumerate(mo["classes"][q]) if c == FRESH)
    assert mo["count"][4] == fresh_bytes
    md, _ = T.model_delta_and_patch([s.model() for s in same], new.model(), one, B, new.nbt, True)
    delta = Spliced(new.dev, new.n, new.nbt, len(md["packed"]) + 32, True)
    sp = m.BlockSplicer.for_extents(gpu_ctx, B, 1, new.n, new.nbt, new.nbt)
    delta.run(sp, [new.view()], outs["delta_first"], outs["delta_ext"])
    gpu_ctx.stream.synchronize()
    sp.close()
    delta.against(md, "delta")
    d = delta.as_built()
    # the read recipe: every extent by a ranged decode of its source, in that source's codec
    srcs = [(FMTS[f], s.packed, s.first, s.off, s.lens) for f, s in zip(fm, stores)]
    nd = int(d["first"][new.n])
    srcs.append((FMTS["lznt1"], bytes(d["packed"][: int(d["off"][nd])]), d["first"], d["off"][: nd + 1], d["new_len"]))
    for q in range(new.n):
        data = b""
        for s, r, k0, c in mo["patch_ext"][mo["patch_first"][q]: mo["patch_first"][q + 1]]:
            f, packed, first, off, lens = srcs[s]
            out, st = m.blocks_decompress(f, packed, first, off, lens, B, ranges=[(k0, c) if x == r else (0, 0) for x in range(len(lens))], ctx=gpu_ctx)
            assert st[r] == 0
            data += out[r]
        assert data == nb[q], q


# ---- 3. payload absent ------------------------------------------------------------------------------------------------------------------
def test_payload_absent(gpu_ctx, cons):
    store, _ = pair(gpu_ctx, cons, "xpress", "recipes")
    new, _ = pair(gpu_ctx, cons, "xpress", "moved")
    mo, outs = check([store], new)
    seen = outs.pull()
    mo2, outs2 = check([store], new, payload=False)                                # d_packed null in both views, the true packed_len
    assert outs2.pull() == seen
    # a packed_len too small refuses exactly the resources rule 3 names: those with a row that ends beyond it
    cut = int(store.off[int(store.first[7])]) + 1
    short = Side(store, plen=cut)
    mo3, _ = check([short], new, payload=False)
    bad = [r for r in range(store.n) if store.blocks(r) and int(store.off[int(store.first[r + 1])]) > cut]
    assert bad and len(bad) < store.n and mo3["status"] == [M.DATA if r in bad else 0 for r in range(store.n)] + [0] * new.n
    mo4, _ = check([store], Side(new, plen=new.plen - 1), payload=False)
    assert mo4["status"][store.n:].count(M.DATA) == 1 and mo4["status"][: store.n] == [0] * store.n


# ---- 4. equality is the digest's alone ---------------------------------------------------------------------------------------------------
def test_equality_is_the_digests_alone(gpu_ctx):
    x, y, z, t = rand(5, B), rand(6, B), rand(7, B), rand(8, 100)
    store = recol(raw_con(gpu_ctx, [x + y, z + t], crc=0x1111), ids(1, 2, 3, 4))
    new = recol(raw_con(gpu_ctx, [y + x, x + t, z[:100]], crc=0x2222), ids(1, 9, 2, 3, 3))
    mo, outs = check([store], new)                                                 # the CRC columns differ between the views
    # y with x's digest is x; x with another digest is fresh; x with y's digest is y; t with z's digest is not z (short against full);
    # z[:100] with z's digest is not z either, but it is the t above it: equal words, equal data length
    assert mo["classes"] == [[FOUND, FRESH], [FOUND, FRESH], [SHARED]]
    assert mo["patch_ext"] == [(0, 0, 0, 1), (1, 0, 0, 1), (0, 0, 1, 1), (1, 1, 0, 1), (1, 1, 0, 1)] and mo["count"] == [2, 1, 2, 5, B + 100, 0]
    for sc, nc in ((False, True), (True, False), (False, False)):                 # a null d_block_crc in some views and not in others
        mo2, outs2 = check([Side(store, sc)], Side(new, nc))
        assert outs2.pull() == outs.pull()
    same_bytes = recol(raw_con(gpu_ctx, [x + y]), ids(7, 8))                       # equal bytes, different digests: not equal
    mo, _ = check([store], same_bytes)
    assert mo["classes"] == [[FRESH, FRESH]]
    full = recol(raw_con(gpu_ctx, [t]), ids(3))                                    # a short block is never represented by a full one with its words
    mo, _ = check([store], full)
    assert mo["classes"] == [[FRESH]] and mo["count"][5] == 0
    mo, _ = check([store], recol(full, ids(4)))                                    # ... and is by a short one of its data length
    assert mo["patch_ext"] == [(0, 1, 1, 1)]


# ---- 5. refuted chain ---------------------------------------------------------------------------------------------------------------------
def test_refuted_chain(gpu_ctx):
    """columns that share (e, h0, h1) in groups and differ in h2 or h3: several distinct rows in one slot, equal ones among the later ones,
    a refuted row equal to an earlier refuted row"""
    k = lambda a, b, g=9: (g, g, a, b)
    store = recol(tab_con(gpu_ctx, [3 * B, 2 * B]), ids(k(0, 0), k(1, 0), k(0, 1), k(0, 0, 4), k(5, 5, 4)))
    new = recol(tab_con(gpu_ctx, [5 * B + 1, 3 * B]), ids(k(1, 0), k(2, 2), k(0, 0), k(2, 2), k(0, 1), k(2, 2), k(5, 5, 4), k(6, 6, 4), k(6, 6, 4)))
    mo, outs = check([store], new, payload=False)
    assert mo["rep"] == [0, 1, 2, 3, 4, 1, 6, 0, 6, 2, 10, 4, 12, 12]
    assert mo["count"] == [4, 2, 3, 9, 21, 10] and mo["classes"] == [[FOUND, FRESH, FOUND, SHARED, FOUND, FRESH], [FOUND, FRESH, SHARED]]
    rebuilt = rebuild_lists(mo)
    assert rebuilt == [[1, 6, 0, 6, 2, 10], [4, 12, 12]]
    mo, _ = check([], new, payload=False)                                          # the chain inside one container
    assert mo["rep"] == [0, 1, 2, 1, 4, 5, 6, 7, 7] and mo["count"][5] == 6


def rebuild_lists(mo):
    """the representatives the patch list names, per resource of next, from the model's own numbering (a check of the test's reading)"""
    u0 = sum(1 for g, _ in mo["rows"] if g < mo["n_store"])
    out, u = [], u0
    for cl in mo["classes"]:
        out.append([mo["rep"][u + i] for i in range(len(cl or []))])
        u += len(cl or [])
    return out


# ---- 6. tiles -----------------------------------------------------------------------------------------------------------------------------
def test_tiles_and_grid_passes(gpu_ctx):
    """next of 2 TILE + 3 rows with a found run across both tile borders, a class change exactly on a border and a shared run whose
    representatives lie in another tile; a store of more rows than one pass of the keys' fixed grid covers (1024 workgroups of 256 lanes
    at most), next's representatives among its last rows. Hand-made tables, made-up columns, no payload"""
    rows = 2 * TILE + 3
    big = 1024 * 256 + 5 * TILE + 77
    sid = np.arange(big, dtype=np.uint32) + 100
    store = recol(tab_con(gpu_ctx, [big * B]), np.stack([sid, sid * 3, sid ^ 0xABCD, sid + 7], axis=1))
    base = big - rows + 100                                                         # store rows from here on are what next holds
    fresh = 10_000_000 + np.arange(10, dtype=np.uint32)
    tail = rows - (TILE + 6)
    nid = np.concatenate([fresh, sid[base + 10: base + TILE], fresh[2:8], sid[base + 100: base + 100 + tail]])
    assert len(nid) == rows
    new = recol(tab_con(gpu_ctx, [rows * B]), np.stack([nid, nid * 3, nid ^ 0xABCD, nid + 7], axis=1))
    mo, outs = check([store], new, payload=False)
    assert mo["patch_ext"] == [(1, 0, 0, 10), (0, 0, base + 10, TILE - 10), (1, 0, 2, 6), (0, 0, base + 100, tail)] and mo["count"][:3] == [rows - 16, 6, 10]
    assert mo["count"][5] == 0
    mo, outs = check([], new, payload=False)                                        # no store: a shared run whose representatives lie a tile back
    assert mo["patch_ext"] == [(0, 0, 0, TILE), (0, 0, 2, 6), (0, 0, 100, TILE - 100), (0, 0, TILE, tail - (TILE - 100))]


# ---- 7. damaged tables ----------------------------------------------------------------------------------------------------------------------
def test_damaged_tables(gpu_ctx, cons):
    """test_gpu_match.py's cases of rules 1-4: the statuses are match's, and no digest of a refused resource is read -- its part of the
    column holds the digests of healthy rows, which would be found there if it were"""
    fmt = "xpress"
    bufs = [rand(41, 2 * B), rand(42, 3 * B + 17), rand(43, B), b"", soft(44, B + 1)]
    good = cons((fmt, "damage"), lambda: with_col(Container.via_host(gpu_ctx, FMTS[fmt], B, bufs), bufs))
    n, lens = good.n, good.lens
    falling = good.first.copy(); falling[1] = falling[2] + np.uint64(1)
    odd = list(lens); odd[1] += B
    j = int(good.first[1])
    back = good.off.copy(); back[j + 2] = back[j + 1] - np.uint64(1)
    last = int(good.off[int(good.first[4])])
    hurt = {"falling": (Side(good.edited(first=falling)), {1: M.ARG, 0: M.DATA}), "odd": (Side(good.edited(lens=odd)), {1: M.DATA}),
            "back": (Side(good.edited(off=back)), {1: M.DATA}), "short": (Side(good, plen=last + 1), {4: M.DATA})}
    blocks = [good.blocks(r) for r in range(n)]
    for name, (con, bad) in hurt.items():
        poisoned = good.dig.copy()
        for r in bad:                                                            # the refused resources' rows say "I am block 0 of resource 2"
            poisoned[int(good.first[r]): int(good.first[r + 1])] = good.dig[int(good.first[2])]
        con = recol(con, poisoned)
        mm, _ = TM.check_match([con], good)
        mo, outs = check([con], good)                                              # a refused store resource brings no rows: its blocks are fresh
        assert mo["status"] == mm["status"] == [bad.get(r, 0) for r in range(n)] + [0] * n, name
        assert mo["cls"] == [x for r in range(n) for x in ((0, 0, blocks[r]) if r in bad else (blocks[r], 0, 0))], name
        assert mo["patch_ext"][mo["patch_first"][2]: mo["patch_first"][3]] == [(0, 2, 0, 1)], name      # not found in a poisoned row, which is smaller
        assert not [1 for s, jj in mo["read"] if s == 0 and any(int(good.first[r]) <= jj < int(good.first[r + 1]) for r in bad)]
        rebuild([con], good, mo, outs)
        mm, _ = TM.check_match([good], con)
        mo, outs = check([good], con)                                              # a refused resource of new: no extents, zero counts
        assert mo["status"] == mm["status"] == [0] * n + [bad.get(r, 0) for r in range(n)], name
        assert [e[1] for e in mo["patch_ext"]] == [r for r in range(n) if lens[r] and r not in bad] and mo["count"][1:3] == [0, 0], name
        rebuild([good], con, mo, outs)
    # rule 4, as match's test builds it
    x = rand(45, 2 * B)
    one = raw_con(gpu_ctx, [x, b"", x])
    twice = recol(Side(one.edited(first=np.array([0, 2, 0, 2], dtype=np.uint64)), nbt=2, plen=2 * B), ids(1, 2))
    store = recol(Side(raw_con(gpu_ctx, [rand(46, B)]), nbt=1), ids(3))
    for total, room, want in ((5, 4, 0), (5, 3, M.ARG), (4, 4, M.ARG), (3, 2, M.ARG)):
        mm, _ = TM.check_match([store], twice, total=total, room=room)
        mo, outs = check([store], twice, total=total, room=room)
        assert mo["status"] == mm["status"] == [0, 0, M.ARG, want] and mo["classes"][2] == (None if want else [SHARED, SHARED]), (total, room)
    mo, outs = check([twice], store, total=3, room=1)
    assert mo["status"] == [0, M.ARG, M.ARG, M.ARG] and mo["count"][:4] == [0, 0, 0, 0]


# ---- 8. degenerate ------------------------------------------------------------------------------------------------------------------------
def test_degenerate(gpu_ctx, cons):
    import torch
    import ms_compress_amd as m
    new, _ = pair(gpu_ctx, cons, "lznt1", "moved")
    mo, outs = check([], new)                                                      # n_src = 0: single-instancing, match's answer with no store
    mm, mouts = TM.check_match([], new)
    got, want = outs.pull(), mouts.pull()
    assert mo["count"][1] > 0 and got["count"][:5] == want["count"][:5] and all(got[k] == want[k] for k in got if k != "count")
    rebuild([], new, mo, outs)
    bufs = [rand(61, B + 5), rand(62, 3 * B)]
    some = with_col(raw_con(gpu_ctx, bufs), bufs)
    none = with_col(Container.from_host(gpu_ctx, 3, B, b"", [0], [0], [], []), col=np.zeros((0, 4), dtype=np.uint32))
    mo, outs = check([some], none)                                                  # an empty new container
    assert mo["count"] == [0] * 6 and mo["delta_first"] == [0] and mo["patch_first"] == [0]
    mo, outs = check([none, none, none], some)                                      # stores without a resource
    assert mo["count"][:4] == [0, 0, 5, 5]
    rebuild([none, none, none], some, mo, outs)
    mo, outs = check([some], Side(some, nbt=0), room=0)                             # n_blocks_new = 0
    assert mo["status"] == [0, 0, M.ARG, M.ARG] and mo["count"] == [0] * 6
    mo, outs = check([some], some)                                                  # next equal to a store: all found, D has no rows
    assert mo["count"][:5] == [5, 0, 0, 5, 0] and mo["delta_ext"] == [] and mo["patch_ext"] == [(0, 0, 0, 2), (0, 1, 0, 3)]
    rebuild([some], some, mo, outs)
    hollow = with_col(raw_con(gpu_ctx, [b"", rand(63, B), b""]), [b"", rand(63, B), b""])   # empty resources between others
    mo, outs = check([hollow], hollow)
    assert mo["cls"] == [0, 0, 0, 1, 0, 0, 0, 0, 0]
    d0 = m.BlockDigestMatcher(gpu_ctx, B, 0, 0, 0, 0)                              # n_res_total = 0: d_count alone is required
    cnt = torch.full((6,), SENT, dtype=torch.int64, device=some.dev)
    d0.match([], [], bare(none.view()), None, None, None, None, None, None, cnt, None)
    gpu_ctx.stream.synchronize()
    assert cnt.cpu().tolist() == [0] * 6
    d0.close()


def busy(gpu_ctx, cons, fmt):
    """match's busy case with true columns, and a refuted chain made in the column of next's resource 2"""
    stores, new = TM.busy_case(gpu_ctx, cons, fmt)
    bufs = R.buffers(B)
    x1 = rand(21, B)
    from dedup_model import crc_twin
    x2, x3 = crc_twin(x1, 1000), crc_twin(x1, 2000)
    data = ([bufs[5], bufs[7], x1 + x2], [bufs[9], bufs[4], bufs[8]],
            [rand(71, B) + bufs[7], bufs[9][B: 3 * B] + rand(72, 2 * B) + bufs[4], x2 + x3 + x3, b"", bufs[8], rand(72, 2 * B)])
    s0, s1, nw = (with_col(c, b) for c, b in zip(stores + [new], data))
    col = nw.dig.copy()
    j = int(nw.first[2])
    col[j + 1] = col[j]; col[j + 1][3] ^= 1                                         # x3: x2's key, another digest
    col[j + 2] = col[j + 1]
    return [s0, s1], recol(nw, col)


# ---- 9. five executions -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FMTS))
def test_five_executions_are_identical(gpu_ctx, cons, fmt):
    """the first execution launches, the later ones replay the object's graph; a changed field of a view or another digest pointer
    captures again"""
    import ms_compress_amd as m
    stores, new = busy(gpu_ctx, cons, fmt)
    room, total, n_all = new.nbt + 3, stores[0].nbt + stores[1].nbt + new.nbt + 5, stores[0].n + stores[1].n + new.n + 2
    dd = m.BlockDigestMatcher(gpu_ctx, B, 2, n_all, total, room)
    outs = Outs(new.dev, new.n, n_all - 2, room)
    seen = []
    for _ in range(5):
        mo, _ = check(stores, new, total=total, room=room, dd=dd, outs=outs)
        seen.append(outs.pull())
    assert mo["count"][5] == 2 and mo["status"] == [0, 0, 0, 0, 0, M.DATA, 0, 0, 0, M.DATA, 0, 0]
    assert mo["count"][:3] == [9, 3, 8] and all(s == seen[0] for s in seen)
    other = new.dig.copy(); other[0] = stores[0].dig[0]                            # another column at another address: row 0 of next is now found
    mo2, _ = check(stores, recol(new, other), total=total, room=room, dd=dd, outs=outs)
    assert mo2["count"][:3] == [10, 3, 7] and outs.pull() != seen[0]
    mo3, _ = check(stores, Side(new, plen=new.cap - 1), total=total, room=room, dd=dd, outs=outs)      # one field of one view
    assert mo3["status"][-1] == M.DATA and mo3["status"][:-1] == mo["status"][:-1]
    check(stores, new, total=total, room=room, dd=dd, outs=outs, payload=False)
    assert outs.pull() == seen[0]
    dd.close()


# ---- 10. capture --------------------------------------------------------------------------------------------------------------------------
def test_match_and_both_splices_in_one_captured_graph():
    """match by digest, the delta splice and the patch splice, all executed for the first time inside one capture of the ctx stream; the
    graph is replayed on the containers it was captured with and on a second set of the same bounds, loaded into the same device arrays"""
    import torch
    import ms_compress_amd as m
    f = FMTS["lznt1"]
    s = torch.cuda.Stream()
    ctx = m.Context(stream=s)
    with torch.cuda.stream(s):
        a = [recipe("text", 4, 6, 33, B), recipe("random", 5, 2, 0, B)]
        b = [recipe("mixed", 31, 6, 33, B), recipe("text", 33, 2, 0, B)]
        fresh = rand(91, B)
        shape = lambda src: [src[1] + src[0][: 2 * B], fresh + src[0][2 * B: 4 * B] + fresh]
        sets = [[with_col(Container.via_host(ctx, f, B, bufs), bufs) for bufs in (src, shape(src))] for src in (a, b)]
        cap = max(c.plen for p in sets for c in p) + 100
        slots = [with_col(Container.from_host(ctx, f, B, c.packed, c.first, c.off, c.lens, c.crc, cap=cap), col=c.dig) for c in sets[0]]
        n, room, n_all = slots[1].n, slots[1].nbt, slots[0].n + slots[1].n
        outs = Outs(slots[1].dev, n, n_all, room)
        dd = m.BlockDigestMatcher(ctx, B, 1, n_all, slots[0].nbt + room, room)
        s1, s2 = m.BlockSplicer.for_extents(ctx, B, 1, n, room, room), m.BlockSplicer.for_extents(ctx, B, 2, n, room, room)
        delta, built = Spliced(slots[1].dev, n, room, cap, True), Spliced(slots[1].dev, n, room, cap, True)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        dd.match([bare(slots[0].view())], [slots[0].d_dig], bare(slots[1].view()), slots[1].d_dig, *outs.tensors())
        delta.run(s1, [slots[1].view()], outs["delta_first"], outs["delta_ext"])
        built.run(s2, [slots[0].view(), delta.view()], outs["patch_first"], outs["patch_ext"])
    for k, (store, new) in enumerate((sets[1], sets[0])):                          # replayed twice
        with torch.cuda.stream(s):
            for slot, con in zip(slots, (store, new)):
                slot.d_packed.fill_(0x3C); slot.d_packed[: con.plen] = con.d_packed[: con.plen]
                slot.d_first.copy_(con.d_first); slot.d_boff.copy_(con.d_boff); slot.d_crc.copy_(con.d_crc); slot.d_dig.copy_(con.d_dig)
            outs.reset(); delta.fill(); built.fill()
            g.replay()
        s.synchronize()
        held = [Container.from_host(ctx, f, B, c.packed + b"\x3C" * (cap - c.plen), c.first, c.off, c.lens, c.crc).model() for c in (store, new)]
        mo = G.model_match_digest(held[:1], [store.dig], held[1], new.dig, B, slots[0].nbt + room, room)
        TM.against_model(outs.pull(), mo)
        assert mo["count"][:3] == [new.blocks(0) + 2, 1, 1], k
        md, mb = T.model_delta_and_patch(held[:1], held[1], mo, B, room, True)
        delta.against(md, "delta, replay %d" % k)
        built.against(mb, "rebuilt, replay %d" % k)
        rebuilt = built.as_built()
        assert bytes(rebuilt["packed"][: new.plen]) == new.packed
    del g
    for h in (dd, s1, s2):
        h.close()
    ctx.close()


# ---- 11. wrong kinds and nulls --------------------------------------------------------------------------------------------------------------
def test_wrong_kinds_and_nulls(gpu_ctx):
    """a matcher refuses dedup, diff, match and repair; the other four kinds refuse match_digest; every array missing in turn; null and
    misaligned columns; views beyond the creation bounds; nothing launched"""
    import torch
    import ms_compress_amd as m
    bufs = [rand(81, 2 * B + 1), rand(82, B)]
    good = with_col(raw_con(gpu_ctx, bufs), bufs)
    n, dev, v = good.n, good.dev, good.view()
    outs = Outs(dev, n, 2 * n, good.nbt)
    full = outs.tensors()
    pairs = d64([0, 0, 1, 1], dev)
    spare = lambda k: torch.full((k,), SENT, dtype=torch.int64, device=dev)
    ver = torch.zeros(good.nbt + 1, dtype=torch.int32, device=dev)
    lib = m.match_digest.bind(gpu_ctx.lib)
    views = m.api._blocks_views([v, v])
    ptrs = [C.c_void_p(t.data_ptr()) for t in full]
    cols = (C.c_void_p * 1)(good.d_dig.data_ptr())
    nd = C.c_void_p(good.d_dig.data_ptr())
    raw = lambda h, store=views, sd=cols, nxt=C.byref(views[1]), dg=nd, out=ptrs: lib.mscomp_amd_deduper_match_digest(h, store, sd, nxt, dg, *out)
    dm = m.BlockDigestMatcher(gpu_ctx, B, 1, 2 * n, 2 * good.nbt, good.nbt)
    others = {"dedup": m.BlockDeduper(gpu_ctx, B, 1, 2 * n, 2 * good.nbt), "diff": m.BlockDeduper.for_diff(gpu_ctx, B, n, good.nbt),
              "match": m.BlockDeduper.for_match(gpu_ctx, B, 1, 2 * n, 2 * good.nbt, good.nbt), "repair": m.BlockDeduper.for_repair(gpu_ctx, B, 1, n, good.nbt)}
    for kind, dd in others.items():                                  # the other kinds refuse the new call
        assert raw(dd._h) == m.MSCOMP_ARG_ERROR, kind
    as_old = m.BlockDeduper.__new__(m.BlockDeduper)                  # the matcher's handle under the old wrapper: it refuses the four old calls
    as_old.ctx, as_old._h, as_old.n_src = gpu_ctx, dm._h, 1
    calls = {"dedup": lambda: as_old.dedup([v], spare(2 * n), spare(2 * n), spare(4 * n), outs["count"], outs.status),
             "diff": lambda: as_old.diff(v, v, pairs, outs["delta_first"], outs["delta_ext"], outs["patch_first"], outs["patch_ext"], spare(n), outs["count"], outs.status),
             "match": lambda: as_old.match([v], v, *full),
             "repair": lambda: as_old.repair([v], [ver], outs["delta_first"], outs["delta_ext"], spare(n), spare(n), outs["count"], outs.status)}
    for call, run in calls.items():
        with pytest.raises(m.MSCompError) as e:
            run()
        assert e.value.status == m.MSCOMP_ARG_ERROR, call
    as_old._h = C.c_void_p()                                         # (the matcher destroys it)
    assert raw(None) == m.MSCOMP_ARG_ERROR
    for k in range(len(full)):                                       # every array missing in turn
        with pytest.raises(m.MSCompError) as e:
            dm.match([v], [good.d_dig], v, good.d_dig, *(full[:k] + (None,) + full[k + 1:]))
        assert e.value.status == m.MSCOMP_ARG_ERROR, k
    for broken in (v[:1] + (None,) + v[2:], v[:2] + (None,) + v[3:], v[:3] + (None,) + v[4:]):        # a view without a table
        for a, b in ((broken, v), (v, broken)):
            with pytest.raises(m.MSCompError) as e:
                dm.match([a], [good.d_dig], b, good.d_dig, *full)
            assert e.value.status == m.MSCOMP_ARG_ERROR
    assert raw(dm._h, store=None) == m.MSCOMP_ARG_ERROR and raw(dm._h, sd=None) == m.MSCOMP_ARG_ERROR and raw(dm._h, nxt=None) == m.MSCOMP_ARG_ERROR
    assert raw(dm._h, dg=None) == m.MSCOMP_ARG_ERROR and raw(dm._h, sd=(C.c_void_p * 1)(None)) == m.MSCOMP_ARG_ERROR          # a null column, either side
    assert raw(dm._h, dg=C.c_void_p(nd.value + 4)) == m.MSCOMP_ARG_ERROR and raw(dm._h, sd=(C.c_void_p * 1)(nd.value + 8)) == m.MSCOMP_ARG_ERROR   # misaligned
    for tight in (m.BlockDigestMatcher(gpu_ctx, B, 1, 2 * n - 1, 2 * good.nbt, good.nbt), m.BlockDigestMatcher(gpu_ctx, B, 1, 2 * n, 2 * good.nbt - 1, good.nbt),
                  m.BlockDigestMatcher(gpu_ctx, B, 1, 2 * n, 2 * good.nbt, good.nbt - 1)):
        with pytest.raises(m.MSCompError) as e:
            tight.match([v], [good.d_dig], v, good.d_dig, *full)
        assert e.value.status == m.MSCOMP_ARG_ERROR
        tight.close()
    torch.cuda.synchronize()
    assert outs.untouched()
    assert raw(dm._h) == m.MSCOMP_OK                                 # and the same call with everything in place is taken
    gpu_ctx.stream.synchronize()
    assert not outs.untouched()
    dm.close()
    for dd in others.values():
        dd.close()


# ---- 12. scratch ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ("lznt1",))
def test_scratch_contract(gpu_ctx, cons, fmt):
    """the documented formula is what the scratch report shows, under the deduper's kind; what an execution reads from the scratch it has
    written itself, and no pass touches the slack"""
    import ms_compress_amd as m
    stores, new = busy(gpu_ctx, cons, fmt)
    room, total, n_all = new.nbt + 3, stores[0].nbt + stores[1].nbt + new.nbt + 5, stores[0].n + stores[1].n + new.n
    dd = m.BlockDigestMatcher(gpu_ctx, B, 2, n_all, total, room)
    outs = Outs(new.dev, new.n, n_all, room)
    check(stores, new, total=total, room=room, dd=dd, outs=outs)
    first = outs.pull()
    as_old = m.BlockDeduper.__new__(m.BlockDeduper)                  # the hooks know the object by its kind: a deduper
    as_old.ctx, as_old._h = gpu_ctx, dd._h
    rep = m.api.scratch_report(as_old, 0)
    assert list(rep) == ["tab"] and rep["tab"][0] == 48 * n_all + 40 * total + 4 * room + 64 * ((room + 1023) // 1024) + 848 and rep["tab"][1] >= rep["tab"][0]
    for byte in POISONS:
        assert m.api.scratch_poison(as_old, byte) == 1
        check(stores, new, total=total, room=room, dd=dd, outs=outs)
        assert outs.pull() == first, "after poison 0x%02X" % byte
        rep = m.api.scratch_report(as_old, byte)
        assert rep["tab"][2] == 0, ("slack bytes touched", byte, rep)
    as_old._h = C.c_void_p()                                         # (the matcher destroys it)
    dd.close()


# ---- 13. host conveniences ------------------------------------------------------------------------------------------------------------------
def test_host_conveniences(gpu_ctx):
    import ms_compress_amd as m
    old = [recipe("text", 41, 3, 17, B), recipe("mixed", 42, 2, 0, B), b"", recipe("random", 43, 1, 5, B)]
    extra = recipe("text", 44, 1, 0, B)
    new = [old[3], extra + old[0], b"", old[1] + old[0][: 2 * B], extra]

    def make(f, bufs):
        packed, first, off, st = m.blocks_compress(f, bufs, B, ctx=gpu_ctx)
        bcrc, _ = m.blocks_crc(f, bufs, B, ctx=gpu_ctx)
        return (packed, first, off, [len(b) for b in bufs], bcrc), m.blocks_digest(bufs, B, ctx=gpu_ctx)
    (s3, ds), (n3, dn) = make(3, old), make(3, new)
    want = m.blocks_match([s3], n3, B, ctx=gpu_ctx)
    got = m.blocks_match_digest([s3], n3, B, [ds], dn, ctx=gpu_ctx)
    assert got[:3] == want[:3] and got[3][:5] == want[3][:5] and got[4] == want[4] == [0] * 9 and got[3][:4] == [10, 1, 1, 12]
    hollow = (None,) + tuple(s3[1:4]) + (None,)                                     # the store as tables and a column: packed=None
    assert m.blocks_match_digest([hollow], n3, B, [ds], dn, ctx=gpu_ctx) == got
    assert m.blocks_match_digest([hollow + (len(s3[0]),)], (None,) + tuple(n3[1:]), B, [ds], dn, ctx=gpu_ctx) == got
    (s4, ds4), _ = make(4, old), None                                               # the same store written by another codec: the same answer
    cross = m.blocks_match_digest([(None,) + tuple(s4[1:])], n3, B, [ds4], dn, ctx=gpu_ctx)
    assert (ds4 == ds).all() and cross == got
    delta, patch2, classes2, counts2, st2 = m.blocks_match_digest_delta([hollow], n3, B, [ds], dn, ctx=gpu_ctx)
    assert (patch2, classes2, counts2, st2) == got[1:] and len(delta[0]) == got[3][4] < len(n3[0])
    packed, first, off, lens, crc, status = m.blocks_match_patch([s3], delta, patch2, B, ctx=gpu_ctx)
    assert status == [0] * 5 and bytes(packed) == bytes(n3[0]) and (off == n3[2]).all() and (crc == n3[4]).all()
    single = m.blocks_match_digest([], n3, B, [], dn, ctx=gpu_ctx)                  # no store: single-instancing
    assert single[:3] == m.blocks_match([], n3, B, ctx=gpu_ctx)[:3]
    with pytest.raises(ValueError):
        m.blocks_match_digest([s3], n3, B, [], dn, ctx=gpu_ctx)
