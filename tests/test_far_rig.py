"""CPU: tests/far_rig.py pinned without a device. FarBytes; the window, guard and alias arithmetic at every base and for every case
geometry the GPU tests use (disjoint, inside the arena, straddling at "2g" and "4g"); every model the far GPU tests call, run on a far
container with the oracle: the input-side offsets shifted by the base, everything else what the model says of the near container -- so the
expected values of the GPU tests are the reference's, and the reference alone passes every case; and the coverage list: every executing
entry point of ms_compress_amd/_abi.py that takes a device offset column or a container view is reached by a far test, or exempt."""
import copy
import zlib

import numpy as np
import pytest

import blocks_model as M
import crc_model as K
import dedup_model as D
import diff_model as F
import digest_model as G
import extents_model as X
import match_model as T
import parity_model as PM
import read_model as R
import repair_model as P
import resize_model as Z
import splice_model as S
import sync_model as Y
import transcode_model as TC
import write_model as W
import far_rig as FR
import plans_rig as PR
from blocks_rig import Container, sources
from parity_rig import lose_host

FMTS = PR.FMTS
B = 4096


# ---- FarBytes -----------------------------------------------------------------------------------------------------------------------------------
def test_far_bytes():
    fb = FR.FarBytes(1000, b"abcdef")
    assert len(fb) == 1006 and fb[1000:1006] == b"abcdef" and fb[1002:1004] == b"cd" and fb[1006:1006] == b"" and fb[1000:1000] == b""
    assert fb[np.uint64(1001): np.uint64(1003)] == b"bc"
    for s in (slice(999, 1002), slice(1004, 1007), slice(0, 6), slice(None, 1003), slice(1001, None), slice(1000, 1006, 2), slice(1003, 1001)):
        with pytest.raises(IndexError):
            fb[s]
    for read in (lambda: fb[1000], lambda: bytes(fb), lambda: list(fb), lambda: fb + b"x"):
        with pytest.raises(TypeError):
            read()


# ---- windows --------------------------------------------------------------------------------------------------------------------------------------
def test_bases_and_places():
    assert FR.ARENA_BYTES == (1 << 32) + (1 << 26)
    assert FR.BASES == {"2g": (1 << 31) - 2051, "4g": (1 << 32) - 2053, "above": (1 << 32) + 4099}
    assert all(b % 2 == 1 for b in FR.PLACES.values()) and FR.PLACES["above+"] > FR.PLACES["above"] > 1 << 32
    assert FR.alias_bases(FR.BASES["2g"]) == [] and FR.alias_bases(FR.BASES["4g"]) == [(1 << 31) - 2053]
    assert FR.alias_bases(FR.BASES["above"]) == [4099] and FR.alias_bases(FR.PLACES["above+"]) == [4099 + (1 << 25)]
    for name in ("2g", "4g"):
        assert FR.straddles(name, FR.BASES[name], FR.FIRST_MIN) and not FR.straddles(name, FR.BASES[name], 2051)
    used_in, used_out = set(), set()
    for pairs in (FR.PAIR, FR.MOVED):
        assert set(pairs) == set(FR.BASES)
        used_in |= {p[0] for p in pairs.values()}
        used_out |= {p[1] for p in pairs.values()}
    assert set(FR.BASES) <= used_in and set(FR.BASES) <= used_out, "every base is an input place and an output place"
    assert all(FR.PAIR[b][0] == b for b in FR.BASES)


def test_window_guards_aliases_and_claims():
    a = FR.HostArena()
    with a.case():
        w = FR.Window(a, FR.BASES["4g"], 5000, "in")
        assert (w.image() == FR.GUARD).all() and w.guards_intact() and w.aliases_intact() and len(w.aliases) == 1
        assert (a.read(w.aliases[0] - FR.EDGE, 5000 + 2 * FR.EDGE) == FR.CANARY).all()
        w.put(10, b"hello")
        w.put_alias(10, b"decoy")
        assert bytes(w.get(10, 5)) == b"hello" and bytes(a.read(w.aliases[0] + 10, 5)) == b"decoy"
        assert w.guards_intact([(10, 5)]) and w.aliases_intact()
        with pytest.raises(AssertionError):
            w.guards_intact([(10, 4)])
        a.write(w.aliases[0] + 3, b"\x00")                                       # a cut store: the canary is touched
        with pytest.raises(AssertionError):
            w.aliases_intact()
        a.write(w.base + 5000, b"\x00")                                          # a byte behind the window
        with pytest.raises(AssertionError):
            w.guards_intact([(10, 5)])
        for base, room in ((FR.BASES["2g"], 5000),                               # where the 31-bit alias of the first window lies
                           ((1 << 32) + 1001, 100),                              # inside the first window
                           (FR.BASES["4g"] + 5000 + FR.EDGE - 1 + FR.EDGE, 10),    # one byte into its upper guard
                           (FR.ARENA_BYTES - 100, 100), (10, 100)):                # the upper guard past the arena; the lower guard in front of it
            with pytest.raises(AssertionError):
                FR.Window(a, base, room)
        n = len(a.claims)
        FR.Window(a, FR.BASES["4g"] + 5000 + 2 * FR.EDGE, 10)                    # guard to guard: fits, and its alias (above 2^32) too
        assert len(a.claims) == n + 2 == 4
    assert a.claims == []
    with a.case():
        FR.Window(a, FR.BASES["2g"], 5000)                                        # the claims of a finished case are given back


@pytest.mark.parametrize("base", list(FR.BASES))
@pytest.mark.parametrize("fmt", list(FMTS))
def test_plan_case_geometry(oracle, fmt, base):
    """the batches of tests/test_gpu_far_plans.py at both pairs of places of the base: windows, guards and aliases disjoint and inside
    the arena (the constructors assert it), the first unit straddling on either side, the decoy other bytes of the same layout"""
    import ms_compress_amd as m
    f = FMTS[fmt]
    plain, comp, decoys = FR.streams(oracle, f)
    assert [len(u) for u in plain] == [70000, 4097, 300, 1, 0] and [len(d) for d in decoys] == [len(c) for c in comp]
    batches = [(PR.layout(plain, caps), PR.layout(FR.units(2), caps)) for caps in [[m.max_compressed_size(f, len(u)) + 2 for u in plain]]]
    batches += [(PR.layout(comp, caps), PR.layout(decoys, caps)) for caps in ([cap(len(p)) for p in plain] for cap in FR.CAPS.values())]
    for near, decoy in batches:
        assert (near.in_off == decoy.in_off).all() and bytes(near.blob) != bytes(decoy.blob)
        for pin, pout in (FR.PAIR[base], FR.MOVED[base]):
            a = FR.HostArena()
            run = FR.FarRun(a, near, FR.PLACES[pin], FR.PLACES[pout], decoy.blob)
            assert run.intact() and run.wout.guards_intact()
            b = run.batch
            assert (b.in_off - near.in_off == FR.PLACES[pin]).all() and int(b.out_off[0]) == FR.PLACES[pout]
            assert (np.diff(b.out_off.astype(np.int64)) == np.diff(near.out_off.astype(np.int64))).all()
            assert all(int(o) % 2 == 1 for o in b.in_off) and int(b.out_off[0]) % 2 == 1
            for name, at, n in ((pin, b.in_off[0], near.lens[0]), (pout, b.out_off[0], near.caps[0])):
                assert name.startswith("above") or FR.straddles(name, int(at), int(n))
            for i, o in enumerate(near.in_off):                                   # a cut offset reads the decoy
                for alias in run.win.aliases:
                    assert bytes(a.read(alias + int(o), int(near.lens[i]))) == bytes(decoy.blob[int(o): int(o) + int(near.lens[i])])


# ---- containers on the host, as Container.make leaves them -------------------------------------------------------------------------------------
def host_container(oracle, f, B, bufs, cls=Container):
    """a blocks_rig.Container from the container model, its device tensors on the CPU"""
    import torch
    packed, plen, first, off, lens, crc, n, nbt = X.source(oracle, f, B, bufs)
    c = cls.__new__(cls)
    c.m, c.ctx, c.fmt, c.B, c.with_crc, c.bk, c.bufs, c.dev = None, None, f, B, True, None, bufs, torch.device("cpu")
    c.packed, c.first, c.off, c.lens, c.n, c.nbt = bytes(packed), first, off, lens, n, nbt
    c.total, c.plen, c.cap, c.crc = sum(lens), plen, plen, crc
    return c


_made = {}


def near_of(oracle, f, B, name="store"):
    bufs = {"store": lambda: FR.store_buffers(B), "second": lambda: FR.store_buffers(B, FR.SECOND), "edited": lambda: FR.edited_buffers(B),
            "collision0": lambda: FR.collision_buffers(B)[0], "collision1": lambda: FR.collision_buffers(B)[1]}
    if (f, B, name) not in _made:
        _made[f, B, name] = host_container(oracle, f, B, bufs[name]())
    return _made[f, B, name]


same = FR.same


def shifted(rows, col, by):
    return [tuple(x + by if i == col else x for i, x in enumerate(r)) for r in rows]


@pytest.fixture(params=[(f, b) for f in FMTS for b in FR.BASES], ids=lambda p: "%s-%s" % p)
def pair(request, oracle):
    """(format, near store, near second, arena, far store at the base's input place, far second at its output place)"""
    fmt, base = request.param
    f = FMTS[fmt]
    n0, n1 = near_of(oracle, f, B), near_of(oracle, f, B, "second")
    a = FR.HostArena()
    return f, n0, n1, a, FR.far_of(oracle, a, n0, FR.PAIR[base][0]), FR.far_of(oracle, a, n1, FR.PAIR[base][1]), base


def test_far_container(pair, oracle):
    """Container.far: the tables but off are shared, off is shifted, cap = plen = base + the stored length, model() gives a FarBytes; the
    decoy is a container of the same table with other contents"""
    f, n0, n1, a, f0, f1, base = pair
    at = FR.PLACES[FR.PAIR[base][0]]
    assert f0.base == at and (f0.off - n0.off == at).all() and f0.cap == f0.plen == at + n0.plen and f0.first is n0.first and f0.lens is n0.lens
    packed, plen, first, off, lens, crc, n, nbt = f0.model()
    assert isinstance(packed, FR.FarBytes) and len(packed) == plen == f0.cap and packed[int(off[0]): int(off[1])] == n0.packed[: int(n0.off[1])]
    assert (f0.model(plen=f0.cap + 9)[0].data, f0.model(plen=f0.cap - 9)[0].data) == (n0.packed + bytes(9), n0.packed[:-9])
    assert n0.base == 0 and n0.model()[0] == n0.packed
    assert FR.settled(f0, f1)
    decoy = FR.decoy_stored(oracle, n0)
    got, st = M.model_decompress(oracle, f, decoy, n0.plen, n0.first, n0.off, n0.lens, B, n0.total, n0.lens)
    assert len(decoy) == n0.plen and all(g != b for g, b in zip(got, n0.bufs)) and 0 in st
    for alias in f0.win.aliases:
        assert bytes(a.read(alias, n0.plen)) == decoy


def test_container_models_on_a_far_container(pair, oracle):
    """blocks_model's decompress, crc_model's check inputs, read_model, write_model, resize_model"""
    f, n0, _, _, f0, _, _ = pair
    for ranges, short, caps in FR.decode_cases(n0.bufs, B):
        near = M.model_decompress(oracle, f, n0.packed, n0.cap, n0.first, n0.off, n0.lens, B, n0.total, caps, ranges)
        same(M.model_decompress(oracle, f, f0.packed, f0.cap, f0.first, f0.off, f0.lens, B, n0.total, caps, ranges), near)
        assert near[1] == [M.BUF if r == short else 0 for r in range(n0.n)]
    reqs = FR.read_requests(B, n0.n)
    caps, bmax = n0.wants(reqs), n0.budget(reqs)
    near = R.model_read(oracle, f, n0.packed, n0.plen, n0.first, n0.off, n0.lens, B, n0.nbt, reqs, caps, bmax, n0.crc)
    same(R.model_read(oracle, f, f0.packed, f0.plen, f0.first, f0.off, f0.lens, B, f0.nbt, reqs, caps, bmax, f0.crc), near)
    assert near[1].count(0) == len(reqs) - 1 and near[1][6] != 0
    assert n0.layout(caps)[0][0] < 2051 and caps[0] >= FR.FIRST_MIN                # the first output buffer straddles
    reqs, kinds = FR.write_requests(B, n0.n, n0.lens[0])
    srcs = sources(n0, reqs, 21, kinds)
    near = W.model_write(oracle, f, n0.packed, n0.plen, n0.first, n0.off, n0.lens, B, n0.nbt, reqs, srcs, n0.budget(reqs), n0.total, n0.crc)
    same(W.model_write(oracle, f, f0.packed, f0.plen, f0.first, f0.off, f0.lens, B, f0.nbt, reqs, srcs, n0.budget(reqs), n0.total, f0.crc), near)
    assert near["status"].count(0) == len(reqs) - 1 and near["status"][6] != 0 and near["res_status"] == [0] * n0.n
    assert n0.wants(reqs)[0] >= FR.FIRST_MIN
    want = FR.resize_want(n0.lens, B)
    nb = int(n0.first[-1])
    for con in (n0, f0):                                                           # (the table widened as blocks_rig.Resizes widens it)
        con.wide = np.concatenate([con.off[: nb + 1], np.full(Z.SPARE, con.off[nb], dtype=np.uint64)])
    wcrc = np.concatenate([n0.crc[:nb], np.zeros(Z.SPARE, dtype=np.uint32)])
    room = n0.total + 24 * B
    near = Z.model_resize(oracle, f, n0.packed, n0.plen, n0.first, n0.wide, n0.lens, B, nb + Z.SPARE, want, 24, room, wcrc)
    same(Z.model_resize(oracle, f, f0.packed, f0.plen, f0.first, f0.wide, f0.lens, B, nb + Z.SPARE, want, 24, room, wcrc), near)
    assert near["res_status"] == [0] * n0.n and near["new_len"] == want
    cap = int(near["off"][1]) + 1                                                  # new_cap inside the second block: refusals
    short = Z.model_resize(oracle, f, n0.packed, n0.plen, n0.first, n0.wide, n0.lens, B, nb + Z.SPARE, want, 24, cap, wcrc)
    same(Z.model_resize(oracle, f, f0.packed, f0.plen, f0.first, f0.wide, f0.lens, B, nb + Z.SPARE, want, 24, cap, wcrc), short)
    assert M.BUF in short["res_status"]


def test_splice_and_dedup_models_on_far_sources(pair, oracle):
    """splice_model, extents_model, dedup_model (the collision construction too)"""
    f, n0, n1, a, f0, f1, base = pair
    nbt, room = n0.nbt + n1.nbt, 2 * n0.total + 3 * B
    near = S.model_splice([n0.model(), n1.model()], FR.PICKS, B, nbt, room)
    same(S.model_splice([f0.model(), f1.model()], FR.PICKS, B, nbt, room), near)
    assert near["status"] == [0, 0, 0, 0, M.ARG, 0, 0]
    ef, ext = X.flat(FR.EXTENTS)
    near = X.model_splice_extents([n0.model(), n1.model()], ef, ext, B, len(ext), nbt, room)
    same(X.model_splice_extents([f0.model(), f1.model()], ef, ext, B, len(ext), nbt, room), near)
    assert near["status"] == [0, 0, 0, M.ARG, 0, 0] and near["new_len"][2] == 17
    for with_crc in (True, False):
        near = D.model_dedup([n0.model(), n1.model()], B, with_crc, n_res_total=6)
        same(D.model_dedup([f0.model(), f1.model()], B, with_crc, n_res_total=6), near)
        assert near["rep"] == [0, 1, 2, 2, 0, 1] and near["status"] == [0] * 6
    c0, c1 = near_of(oracle, f, B, "collision0"), near_of(oracle, f, B, "collision1")
    with a.case():
        del a.claims[:]                                                            # (the collision pair takes the places of the store pair)
        g0, g1 = FR.far_of(oracle, a, c0, FR.PAIR[base][0]), FR.far_of(oracle, a, c1, FR.PAIR[base][1])
        near = D.model_dedup([c0.model(), c1.model()], B, True, n_res_total=4)
        same(D.model_dedup([g0.model(), g1.model()], B, True, n_res_total=4), near)
        assert near["rep"] == [0, 1, 2, 0] and near["count"][0] == 3 and near["count"][3] == 1 and (c0.crc[:4] == c1.crc[:4]).all()


def test_match_and_diff_models_on_far_sources(pair, oracle):
    f, n0, _, a, f0, _, base = pair
    n1 = near_of(oracle, f, B, "edited")
    del a.claims[1:]                                                               # (the later version takes the place of the second source)
    f1 = FR.far_of(oracle, a, n1, FR.PAIR[base][1])
    total, room = n0.nbt + n1.nbt, n1.nbt
    near = T.model_match([n0.model()], n1.model(), B, total, room, True)
    far = T.model_match([f0.model()], f1.model(), B, total, room, True)
    same(far, near)
    T.holds_consequence([f0.model()], f1.model(), far, B, room, True)
    same(T.model_delta_and_patch([f0.model()], f1.model(), far, B, room, True), T.model_delta_and_patch([n0.model()], n1.model(), near, B, room, True))
    pairs = F.default_pairs(n0.model(), n1.model())
    assert F.default_pairs(f0.model(), f1.model()) == pairs
    room = sum(n1.blocks(b) for _, b in pairs)
    near = F.model_diff(n0.model(), n1.model(), pairs, B, room, True)
    far = F.model_diff(f0.model(), f1.model(), pairs, B, room, True)
    same(far, near)
    same(F.model_delta_and_patch(f0.model(), f1.model(), pairs, far, B, room, True), F.model_delta_and_patch(n0.model(), n1.model(), pairs, near, B, room, True))
    assert near["count"][0] > 0


@pytest.mark.parametrize("case", ["edits", "seams"])
def test_sync_and_digest_models_on_a_far_store(pair, oracle, case):
    """sync_model and digest_model.model_sync_digest: the unit offsets far as well; req_off and the literal offsets move with them"""
    f, n0, _, a, f0, _, base = pair
    units = [bytes(u) for u in Y.cases(B)[case]]
    room = sum(len(u) for u in units)
    nc = 2 * (room // B) + 8
    from blocks_rig import odd_offsets
    offs, _ = odd_offsets(units, room + 3 * len(units) + 64)
    del a.claims[1:]
    w, far_offs, rel = FR.plain_window(a, FR.PAIR[base][1], units, room + 3 * len(units) + 64, "units")
    assert rel == offs
    by = w.base
    dig = G.store_digests(n0.bufs, B, n0.nbt)
    for run in (lambda store, o: Y.model_sync(oracle, f, store, units, o, B, room, nc), lambda store, o: G.model_sync_digest(store, dig, units, o, B, room, nc)):
        near, far = run(n0.model(), offs), run(f0.model(), far_offs)
        assert far["req_off"] == [x + by for x in near["req_off"]] and far["lit"] == shifted(near["lit"], 0, by) and near["req_off"]
        same({k: v for k, v in far.items() if k not in ("req_off", "lit")}, {k: v for k, v in near.items() if k not in ("req_off", "lit")})


@pytest.mark.parametrize("base", list(FR.BASES))
@pytest.mark.parametrize("name,f1,B1,f2,B2", FR.TRANSCODES)
def test_transcode_model_on_a_far_source(oracle, name, f1, B1, f2, B2, base):
    bufs = Y.store_buffers(min(B1, B2) if name != "wide" else B1)
    lens = [len(b) for b in bufs]
    packed, first, off, crc = TC.fresh(oracle, f1, bufs, B1, True)
    nbt, G_ = len(off) - 1, max(B1, B2)
    nbn, gmax = sum((x + B2 - 1) // B2 for x in lens), sum((x + G_ - 1) // G_ for x in lens)
    at = FR.PLACES[FR.PAIR[base][0]]
    FR.Window(FR.HostArena(), at, len(packed), "source")
    assert base == "above" or FR.straddles(base, at + int(off[0]), int(off[1] - off[0]))
    near = TC.transcode(oracle, f1, B1, f2, B2, packed, len(packed), first, off, lens, crc, nbt, nbn, gmax, sum(lens))
    far = TC.transcode(oracle, f1, B1, f2, B2, FR.FarBytes(at, packed), at + len(packed), first, off + np.uint64(at), lens, crc, nbt, nbn, gmax, sum(lens))
    same(far, near)
    assert list(near[4]) == [0] * len(bufs) and (name not in ("join", "split") or near[5][1] > 0 or near[5][2] > 0)


def test_parity_and_repair_models_on_far_sources(pair, oracle):
    """parity_model's build and rebuild; repair_model's salvage, repair and rebuild over a damaged far primary and a healthy far mirror"""
    f, n0, _, a, f0, _, base = pair
    k, m = FR.PARITY
    nb = int(n0.first[-1])
    near = PM.model_build(n0.model(False), B, k, m, 1 << 40, nbt=n0.nbt)
    same(PM.model_build(f0.model(False), B, k, m, 1 << 40, nbt=n0.nbt), near)
    assert near["status"] == 0
    pset = {"par": b"".join(b for _, b in sorted(near["pieces"])), "par_off": np.array(near["par_off"], dtype=np.uint64),
            "par_crc": np.array(near["par_crc"], dtype=np.uint32), "row_len": np.array(near["row_len"], dtype=np.uint32),
            "head": np.array(near["head"], dtype=np.uint64)}
    par_len = int(near["par_off"][-1])
    src, ver = lose_host(n0.model(False), [0, nb - 1])
    dam = copy.copy(n0)
    dam.packed, dam.decoy = src[0][: n0.plen], n0.packed
    del a.claims[:]
    fdam, fmir = FR.far_of(oracle, a, dam, FR.PAIR[base][0]), FR.far_of(oracle, a, n0, FR.PAIR[base][1])
    nfix = PM.model_rebuild(dam.model(False), ver, pset, B, k, m, n0.plen + 64, nbt=n0.nbt, par_len=par_len)
    same(PM.model_rebuild(fdam.model(False), ver, pset, B, k, m, n0.plen + 64, nbt=n0.nbt, par_len=par_len), nfix)
    assert nfix["status"] == 0 and nfix["count"][0] >= 2
    dam.packed = FR.damaged_stored(oracle, n0)
    del a.claims[:]
    fdam, fmir = FR.far_of(oracle, a, dam, FR.PAIR[base][0]), FR.far_of(oracle, a, n0, FR.PAIR[base][1])
    nmo = P.model_salvage(oracle, f, dam.model(), B, n0.total, n0.lens)
    nmi = P.model_salvage(oracle, f, n0.model(), B, n0.total, n0.lens, only=nmo["verdict"])
    mo = P.model_salvage(oracle, f, fdam.model(), B, n0.total, n0.lens)
    mi = P.model_salvage(oracle, f, fmir.model(), B, n0.total, n0.lens, only=mo["verdict"])
    same(mo, nmo); same(mi, nmi)
    assert nmo["bad"][0] == 2
    nro = P.model_repair([dam.model(), n0.model()], [nmo["verdict"], nmi["verdict"]], B, n0.n, nb)
    ro = P.model_repair([fdam.model(), fmir.model()], [mo["verdict"], mi["verdict"]], B, n0.n, nb)
    same(ro, nro)
    assert nro["status"] == [0] * n0.n and nro["count"][1] == 0
    cap = 2 * n0.plen + 32
    built = P.model_rebuild([fdam.model(), fmir.model()], ro, B, n_ext=nb, cap=cap)
    same(built, P.model_rebuild([dam.model(), n0.model()], nro, B, n_ext=nb, cap=cap))
    assert bytes(built["packed"][: n0.plen]) == n0.packed


def test_digest_and_crc_columns_of_the_store(oracle):
    """what the far compress, crc and digester cases expect: the models' columns of the store's data (they take no container)"""
    bufs = FR.store_buffers(B)
    total = sum(len(b) for b in bufs)
    bc, rc, st = K.blocks(bufs, B, total)
    assert [int(x) for x in rc] == [zlib.crc32(b) for b in bufs] and not np.asarray(st).any()
    dig, st = G.model_digests(bufs, B, total)
    assert not np.asarray(st).any() and (dig[: len(bufs) + total // B] == G.store_digests(bufs, B, len(bufs) + total // B)).all()
    assert len(bufs[0]) == 3 * B + 17 and bufs[1] == bytes(5 * B) and len(bufs[2]) == B


# ---- the coverage list ----------------------------------------------------------------------------------------------------------------------------
PLANS, BLOCKS = "test_gpu_far_plans.py::", "test_gpu_far_blocks.py::"
COVERED = {
    "mscomp_amd_plan_execute":              PLANS + "test_compress_at_far_offsets, test_decompress_at_far_offsets (host tables from plan_create / plan_create_decompress)",
    "mscomp_amd_plan_create":               PLANS + "test_compress_at_far_offsets (takes in_off / out_off)",
    "mscomp_amd_plan_create_decompress":    PLANS + "test_decompress_at_far_offsets (takes in_off / out_off)",
    "mscomp_amd_plan_create_size":          PLANS + "test_size_query_at_far_offsets (takes in_off)",
    "mscomp_amd_plan_execute_size":         PLANS + "test_size_query_at_far_offsets",
    "mscomp_amd_plan_execute_dev":          PLANS + "test_compress_at_far_offsets, test_decompress_at_far_offsets",
    "mscomp_amd_plan_execute_size_dev":     PLANS + "test_size_query_at_far_offsets",
    "mscomp_amd_compress_batch":            PLANS + "test_one_shot_batches_at_far_offsets",
    "mscomp_amd_decompress_batch":          PLANS + "test_one_shot_batches_at_far_offsets",
    "mscomp_amd_decompressed_size_batch":   PLANS + "test_size_query_at_far_offsets",
    "mscomp_amd_compact_batch":             PLANS + "test_compaction_at_far_offsets (far out_off)",
    "mscomp_amd_compact_dev":               PLANS + "test_compaction_at_far_offsets (far d_src_off)",
    "mscomp_amd_plan_execute_crc_dev":      PLANS + "test_crc_plan_at_far_offsets",
    "mscomp_amd_blocks_compress":           BLOCKS + "test_compress_and_crc_from_far_resource_offsets",
    "mscomp_amd_blocks_crc":                BLOCKS + "test_compress_and_crc_from_far_resource_offsets",
    "mscomp_amd_blocks_decompress":         BLOCKS + "test_decompress_and_check_into_far_output_offsets",
    "mscomp_amd_blocks_check":              BLOCKS + "test_decompress_and_check_into_far_output_offsets",
    "mscomp_amd_blocks_salvage":            BLOCKS + "test_salvage_and_repair_of_a_far_primary_and_a_far_mirror",
    "mscomp_amd_reader_read":               BLOCKS + "test_reader_from_a_far_container_into_far_output_offsets",
    "mscomp_amd_writer_write":              BLOCKS + "test_writer_on_a_far_container_from_far_source_offsets",
    "mscomp_amd_writer_resize":             BLOCKS + "test_resize_of_a_far_container",
    "mscomp_amd_splicer_splice":            BLOCKS + "test_splices_of_two_far_sources",
    "mscomp_amd_splicer_splice_extents":    BLOCKS + "test_splices_of_two_far_sources",
    "mscomp_amd_deduper_dedup":             BLOCKS + "test_dedup_of_two_far_sources",
    "mscomp_amd_deduper_diff":              BLOCKS + "test_match_and_diff_of_two_far_sources",
    "mscomp_amd_deduper_match":             BLOCKS + "test_match_and_diff_of_two_far_sources",
    "mscomp_amd_deduper_repair":            BLOCKS + "test_salvage_and_repair_of_a_far_primary_and_a_far_mirror",
    "mscomp_amd_transcoder_transcode":      BLOCKS + "test_transcode_of_a_far_source",
    "mscomp_amd_syncer_sync":               BLOCKS + "test_sync_and_sync_digest_of_a_far_store_and_far_units",
    "mscomp_amd_syncer_sync_digest":        BLOCKS + "test_sync_and_sync_digest_of_a_far_store_and_far_units",
    "mscomp_amd_digester_blocks":           BLOCKS + "test_digester_blocks_and_check_at_far_offsets",
    "mscomp_amd_digester_check":            BLOCKS + "test_digester_blocks_and_check_at_far_offsets",
    "mscomp_amd_parity_build":              BLOCKS + "test_parity_build_and_rebuild_of_a_far_container",
    "mscomp_amd_parity_rebuild":            BLOCKS + "test_parity_build_and_rebuild_of_a_far_container",
}
_ONE_SHOT = "a host-pointer one-shot call: one buffer in, one out, no offsets"
_STREAM = "a host-pointer streaming call: no offsets"
_CREATE = "creation from bounds: takes no offsets and executes nothing"
_DESTROY = "destroys an object"
_COUNTS = "reads back an object's counts or bounds"
_HOOK = "a debug or measurement hook: takes no caller offsets"
_SWITCH = "a process- or context-wide switch"
EXEMPT = dict(
    {n: _ONE_SHOT for n in ("ms_compress", "lznt1_compress", "xpress_compress", "xpress_huff_compress", "ms_decompress", "lznt1_decompress",
                            "xpress_decompress", "xpress_huff_decompress")},
    **{n: "a size bound computed on the host" for n in ("ms_max_compressed_size", "lznt1_max_compressed_size", "xpress_max_compressed_size",
                                                         "xpress_huff_max_compressed_size")},
    **{"%s_%s%s" % (c, d, s): _STREAM for c, ds in (("ms", ("deflate", "inflate")), ("lznt1", ("deflate", "inflate")), ("xpress", ("deflate", "inflate")))
       for d in ds for s in ("_init", "", "_end")},
    **{n: _CREATE for n in ("mscomp_amd_ctx_create", "mscomp_amd_plan_create_decompress_dev", "mscomp_amd_plan_create_size_dev",
                            "mscomp_amd_plan_create_decompress_dev_ex", "mscomp_amd_plan_create_size_dev_ex", "mscomp_amd_plan_create_compress_dev",
                            "mscomp_amd_plan_create_crc_dev", "mscomp_amd_blocks_create", "mscomp_amd_reader_create", "mscomp_amd_writer_create",
                            "mscomp_amd_splicer_create", "mscomp_amd_splicer_create_extents", "mscomp_amd_deduper_create", "mscomp_amd_deduper_create_diff",
                            "mscomp_amd_deduper_create_match", "mscomp_amd_deduper_create_repair", "mscomp_amd_transcoder_create", "mscomp_amd_syncer_create",
                            "mscomp_amd_digester_create", "mscomp_amd_syncer_create_digest", "mscomp_amd_parity_create")},
    **{n: _DESTROY for n in ("mscomp_amd_ctx_destroy", "mscomp_amd_plan_destroy", "mscomp_amd_blocks_destroy", "mscomp_amd_reader_destroy",
                             "mscomp_amd_writer_destroy", "mscomp_amd_splicer_destroy", "mscomp_amd_deduper_destroy", "mscomp_amd_transcoder_destroy",
                             "mscomp_amd_syncer_destroy", "mscomp_amd_digester_destroy", "mscomp_amd_parity_destroy", "mscomp_amd_host_pool_release")},
    **{n: _COUNTS for n in ("mscomp_amd_blocks_bound", "mscomp_amd_reader_counts", "mscomp_amd_writer_counts", "mscomp_amd_transcoder_counts",
                            "mscomp_amd_syncer_counts", "mscomp_amd_parity_bound", "mscomp_amd_version")},
    **{n: _HOOK for n in ("mscomp_amd_profile_enable", "mscomp_amd_profile_read", "mscomp_amd_debug_xpress_matches", "mscomp_amd_debug_huff_lengths",
                          "mscomp_amd_debug_huff_lengths_slow", "mscomp_amd_debug_hooks_enabled", "mscomp_amd_debug_lzg_open", "mscomp_amd_debug_lzd_walked",
                          "mscomp_amd_debug_decode_modes", "mscomp_amd_debug_plan_paths", "mscomp_amd_debug_scratch_names", "mscomp_amd_debug_scratch_poison",
                          "mscomp_amd_debug_scratch_report", "mscomp_amd_debug_lds_lane_order", "mscomp_amd_debug_alignbyte")},
    **{n: _SWITCH for n in ("mscomp_amd_debug_set_xpress_emit", "mscomp_amd_set_lznt1_sa_dict", "mscomp_amd_get_lznt1_sa_dict", "mscomp_amd_ctx_set_lznt1_sa_dict",
                            "mscomp_amd_debug_set_xpress_decoder", "mscomp_amd_debug_set_finder", "mscomp_amd_debug_set_one_shot", "mscomp_amd_debug_set_lznt1",
                            "mscomp_amd_debug_set_place_blocks", "mscomp_amd_debug_set_serial_atomics")},
    **{"mscomp_amd_compress_units_host": "host pointers per unit, no offsets", "mscomp_amd_decompress_units_host": "host pointers per unit, no offsets",
       "mscomp_amd_layout_dev": "lengths in, offsets out: the offsets are its own running sums",
       "mscomp_amd_plan_layout_dev": "lengths in, offsets out: the offsets are its own running sums",
       "mscomp_amd_plan_layout": "lengths in, offsets out, on the host",
       "mscomp_amd_res_crc_dev": "folds block checksums by block_first and lengths: reads no byte of a container and takes no byte offset"})


def test_every_entry_point_is_covered_or_exempt():
    from ms_compress_amd import _abi
    import os
    assert not set(COVERED) & set(EXEMPT)
    assert set(COVERED) | set(EXEMPT) == set(_abi.SIGNATURES), (set(_abi.SIGNATURES) - set(COVERED) - set(EXEMPT), (set(COVERED) | set(EXEMPT)) - set(_abi.SIGNATURES))
    assert all(len(reason) > 10 for reason in EXEMPT.values())
    here = os.path.dirname(os.path.abspath(__file__))
    for name, where in COVERED.items():                                            # the tests named exist
        module, _, tests = where.partition("::")
        text = open(os.path.join(here, module)).read()
        for t in tests.split(" (")[0].split(", "):
            assert "def %s(" % t in text, (name, t)
