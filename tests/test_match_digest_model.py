"""CPU: the model of match by digest (tests/match_digest_model.py). The GPU tests compare mscomp_amd_deduper_match_digest with this model
array for array, so the model is pinned here: against a brute-force comparison of the DECODED blocks on seeded inputs (with true digests
the call must say what the data says); against tests/match_model.py wherever both apply (hand-made containers whose blocks are all stored
raw, with checksums: every output but the refuted count); on made-up columns, where equality is the column's alone and the count of the
refuted is known; and with every branch reached: found, shared, fresh, refuted, short last blocks."""
import numpy as np
import pytest

import match_digest_model as G
import match_model as T
from dedup_model import raw_source

FOUND, SHARED, FRESH = T.FOUND, T.SHARED, T.FRESH
SAME = ("status", "cls", "count", "delta_first", "patch_first", "delta_ext", "patch_ext", "rows", "rep", "classes", "n_store")


@pytest.fixture(scope="module", autouse=True)
def api():
    import ms_compress_amd as m                                  # the model describes this library's call: no call, no test
    assert "mscomp_amd_deduper_match_digest" in m.match_digest.EXPORTS


def rand(seed, n):
    return np.random.RandomState(seed).bytes(n)


def blocks_of(bufs, B):
    return sum((len(b) + B - 1) // B for b in bufs)


def both(stores, new, B, spare=2):
    """raw containers of the buffers and their true columns; the digest model, held to match's model in everything but count[5]"""
    srcs, nsrc = [raw_source(b, B, spare) for b in stores], raw_source(new, B, spare)
    cols, ncol = [G.column(b, B, s[7]) for b, s in zip(stores, srcs)], G.column(new, B, nsrc[7])
    room = blocks_of(new, B)
    total = sum(blocks_of(b, B) for b in stores) + room
    d = G.model_match_digest(srcs, cols, nsrc, ncol, B, total, room)
    t = T.model_match(srcs, nsrc, B, total, room, True)
    for k in SAME:
        assert d[k] == t[k] or (k == "count" and d[k][:5] == t[k][:5]), k
    assert d["count"][5] == 0
    G.holds_consequence(srcs, nsrc, d, B, room, True)
    return d


def seeded_case(seed, B):
    """stores and a new container cut from one pool of blocks: repeats inside and across containers, short tails that repeat too"""
    rs = np.random.RandomState(seed)
    pool = [rs.bytes(B) for _ in range(6)] + [rs.bytes(B)[:100], rs.bytes(B)[:B - 1], bytes(B)]
    tails = [b"", pool[6], pool[7], pool[0][:100], bytes(100)]

    def con(n):
        out = []
        for _ in range(n):
            body = b"".join(p for p in (pool[i] for i in rs.randint(0, 9, rs.randint(0, 6))) if len(p) == B)
            out.append(body + tails[rs.randint(0, len(tails))])
        return out
    return [con(rs.randint(1, 4)) for _ in range(rs.randint(0, 4))], con(rs.randint(1, 5))


@pytest.mark.parametrize("seed", range(12))
def test_true_digests_say_what_the_decoded_blocks_say(seed):
    B = 4096
    stores, new = seeded_case(seed, B)
    d = both(stores, new, B)
    want = G.brute_force(stores, new, B)
    n_store = d["n_store"]
    res_of = [(s, r) for s, bufs in enumerate(stores) for r in range(len(bufs))]
    for u, (g, k) in enumerate(d["rows"]):
        if g < n_store:
            continue
        q = g - n_store
        rg, rk = d["rows"][d["rep"][u]]
        got = ("fresh",) if d["rep"][u] == u else ("found",) + res_of[rg] + (rk,) if rg < n_store else ("shared", rg - n_store, rk)
        assert got == want[(q, k)], (seed, q, k)
    assert len(want) == d["count"][3]


def test_every_branch_is_reached():
    B = 4096
    seen = {"found": 0, "shared": 0, "fresh": 0, "short found": 0, "short shared": 0, "short fresh": 0}
    for seed in range(12):
        stores, new = seeded_case(seed, B)
        for (q, k), v in G.brute_force(stores, new, B).items():
            short = len(new[q]) - k * B < B
            seen[("short " if short else "") + v[0]] += 1
    assert all(seen.values()), seen


def test_moves_and_short_blocks():
    B = 4096
    a, b, c, extra = rand(1, 3 * B + 17), rand(2, 2 * B), rand(3, B + 1), rand(4, B)
    d = both([[a, b, c, b""]], [c, extra + a, b"", b + a[: 2 * B], b[B:] + b[:B]], B)
    assert d["count"] == [12, 0, 1, 13, B, 0]
    assert d["patch_ext"] == [(0, 2, 0, 2), (1, 1, 0, 1), (0, 0, 0, 4), (0, 1, 0, 2), (0, 0, 0, 2), (0, 1, 1, 1), (0, 1, 0, 1)]
    x, t = rand(8, B), rand(9, 100)
    d = both([[rand(10, B), x + t], [x, x + t, x[:100]]], [x + t, t, x[:100], x[:50]], B)
    assert d["patch_ext"] == [(0, 1, 0, 2), (0, 1, 1, 1), (1, 2, 0, 1), (2, 3, 0, 1)] and d["count"][:3] == [4, 0, 1]
    d = both([], [t, t, x + t], B)                                                   # no store: equal tails are shared
    assert d["classes"] == [[FRESH], [SHARED], [FRESH, SHARED]]


def made_up(lens_by_con, B, cols):
    """containers of these resource lengths without payload, every stored length 7, and the made-up columns given per container"""
    out = []
    for lens in lens_by_con:
        nb = sum((L + B - 1) // B for L in lens)
        first = np.cumsum([0] + [(L + B - 1) // B for L in lens]).astype(np.uint64)
        off = (np.arange(nb + 1) * 7).astype(np.uint64)
        out.append((None, 7 * nb, first, off, list(lens), None, len(lens), nb))
    return out, [np.array(c, dtype=np.uint32).reshape(-1, 4) for c in cols]


def test_equality_is_the_columns_alone():
    """no payload at all; rows with one digest are one block, whatever they are; a short row is never represented by a full one"""
    B = 4096
    X, Y = (1, 2, 3, 4), (5, 6, 7, 8)
    (store, new), (cs, cn) = made_up([[2 * B], [B + 100, 100, 99]], B, [[X, Y], [Y, X, X, X]])
    d = G.model_match_digest([store], [cs], new, cn, B, 6, 4)
    assert d["classes"] == [[FOUND, FRESH], [SHARED], [FRESH]]                        # X of 100 bytes is not X of B bytes, nor X of 99
    assert d["patch_ext"] == [(0, 0, 1, 1), (1, 0, 0, 1), (1, 0, 0, 1), (1, 2, 0, 1)] and d["count"] == [1, 1, 2, 4, 14, 0]
    assert d["delta_ext"] == [(0, 0, 1, 1), (0, 2, 0, 1)]


def test_refuted_chain():
    """rows that share (e, h0, h1) and differ in h2 or h3: several distinct rows in one slot, equal ones among the later ones, a refuted
    row equal to an earlier refuted row"""
    B = 4096
    k = lambda a, b: (9, 9, a, b)
    (store, new), (cs, cn) = made_up([[3 * B], [5 * B + 1]], B, [[k(0, 0), k(1, 0), k(0, 1)], [k(1, 0), k(2, 2), k(0, 0), k(2, 2), k(0, 1), k(2, 2)]])
    d = G.model_match_digest([store], [cs], new, cn, B, 9, 6)
    assert d["rep"] == [0, 1, 2, 1, 4, 0, 4, 2, 8]                                    # the last row is short: the same words, another key
    assert d["count"] == [3, 1, 2, 6, 14, 6]                                          # refuted: rows 1, 2, 3, 4, 6 and 7; row 5 equals row 0, row 8 has a key of its own
    assert d["classes"] == [[FOUND, FRESH, FOUND, SHARED, FOUND, FRESH]]
    d2 = G.model_match_digest([], [], new, cn, B, 6, 6)                              # the chain inside one container
    assert d2["rep"] == [0, 1, 2, 1, 4, 5] and d2["count"][5] == 4


def test_refused_resources_read_no_digest():
    B = 4096
    (store, new), (cs, cn) = made_up([[B, 2 * B], [B, B]], B, [[(1, 1, 1, 1), (2, 2, 2, 2), (3, 3, 3, 3)], [(2, 2, 2, 2), (1, 1, 1, 1)]])
    bad = store[:4] + ([B, 3 * B],) + store[5:]                                      # rule 2 refuses resource 1 of the store
    d = G.model_match_digest([bad], [cs], new, cn, B, 5, 2)
    assert d["status"] == [0, T.DATA, 0, 0] and d["classes"] == [[FRESH], [FOUND]] and (0, 1) not in d["read"] and (0, 2) not in d["read"]
    short = store[:1] + (7 * 2,) + store[2:]                                         # rule 3: the last row ends beyond packed_len
    d = G.model_match_digest([short], [cs], new, cn, B, 5, 2)
    assert d["status"] == [0, T.DATA, 0, 0]
