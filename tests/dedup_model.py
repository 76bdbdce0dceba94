"""The block deduper (include/mscomp_amd.h, mscomp_amd_deduper_*) restated over plain lists and bytes: which resources of the source
containers hold the same stored bytes, with the header's rules 1-7 in their order, and the count of the refuted from the key tuple as the
header defines it. Dedup never encodes or decodes, so no oracle is called. Not collected as a test.

A source is what splice_model.model_splice takes: (packed, packed_len, block_first, block_off, lengths, block_crc or None, n_res,
n_blocks_table).
"""
import numpy as np

import blocks_model as M
import read_model as R
from splice_model import ORDER2

OK, ARG, DATA = M.OK, M.ARG, M.DATA
M64 = M.M64
PAD = M64                                                      # a pick behind the unique ones: no such source


def judge(source, r, B):
    """(status, rows) of resource r by rules 1-3: rows = [(offset, stored length, row index)] of an accepted resource"""
    packed, plen, first, off, lens, crc, n_res, nbt = source
    f0, f1 = int(first[r]), int(first[r + 1])
    if f0 > f1 or f1 > int(nbt):
        return ARG, None
    L = int(lens[r])
    if f1 - f0 != L // B + (1 if L % B else 0):
        return DATA, None
    rows = []
    for j in range(f0, f1):
        o0, o1 = int(off[j]), int(off[j + 1])
        if not o0 <= o1 <= int(plen):
            return DATA, None
        rows.append((o0, o1 - o0, j))
    return OK, rows


def describe(source, r, rows, with_crc):
    """(what rule 5 compares, the key tuple) of an accepted resource"""
    packed, crc, L = source[0], source[5], int(source[4][r])
    whole = (L, tuple((s, bytes(packed[o: o + s]), int(crc[j]) if with_crc else None) for o, s, j in rows))
    key = (L, tuple((s, int(crc[j]) if with_crc else None, bytes(packed[o: o + min(16, s)]), bytes(packed[o + s - min(16, s): o + s])) for o, s, j in rows))
    return whole, key


def model_dedup(sources, B, with_crc, n_res_total=None):
    """{"rep" [N], "new_index" [N], "pick" [2 n_res_total, padded], "count" [4], "status" [N], "where": (source, resource) of every g}"""
    with_crc = with_crc and all(s[5] is not None for s in sources)
    where = [(s, r) for s, src in enumerate(sources) for r in range(int(src[6]))]
    N = len(where)
    n_res_total = N if n_res_total is None else n_res_total
    assert N <= n_res_total
    status, whole, key = [], [], []
    for s, r in where:
        st, rows = judge(sources[s], r, B)
        w, k = describe(sources[s], r, rows, with_crc) if st == OK else (None, None)
        status.append(st); whole.append(w); key.append(k)
    rep, refuted = [], 0
    for g in range(N):
        if status[g] != OK:                                    # rule 4
            rep.append(g)
            continue
        rep.append(next(h for h in range(g + 1) if status[h] == OK and whole[h] == whole[g]))   # rule 6
        least = next(h for h in range(g + 1) if status[h] == OK and key[h] == key[g])           # the candidate
        if least != g and whole[least] != whole[g]:
            refuted += 1
    unique = [g for g in range(N) if rep[g] == g]
    rank = {g: q for q, g in enumerate(unique)}
    pick = [x for g in unique for x in where[g]] + [PAD] * (2 * (n_res_total - len(unique)))
    saved = sum(sum(s for _, s, _ in judge(sources[where[g][0]], where[g][1], B)[1]) for g in range(N) if rep[g] != g)
    return {"rep": rep, "new_index": [rank[rep[g]] for g in range(N)], "pick": pick, "count": [len(unique), N, saved, refuted],
            "status": status, "where": where}


def holds_consequence(sources, B, with_crc, d, new):
    """the header's consequence: in the container ``new`` spliced from d's picks ({"packed", "first", "off", "crc", "new_len"}, as
    model_splice returns them), resource new_index[g] has the length, the rows, the stored bytes and the CRC words of every accepted g"""
    for g, (s, r) in enumerate(d["where"]):
        if d["status"][g] != OK:
            continue
        packed, crc = sources[s][0], sources[s][5]
        q, rows = d["new_index"][g], judge(sources[s], r, B)[1]
        f0, f1 = int(new["first"][q]), int(new["first"][q + 1])
        assert int(new["new_len"][q]) == int(sources[s][4][r]) and f1 - f0 == len(rows), ("length or rows of", g, "as", q)
        for k, (o, ln, j) in enumerate(rows):
            n0, n1 = int(new["off"][f0 + k]), int(new["off"][f0 + k + 1])
            assert n1 - n0 == ln and bytes(new["packed"][n0:n1]) == bytes(packed[o: o + ln]), ("row", k, "of", g, "as", q)
            assert not with_crc or int(new["crc"][f0 + k]) == int(crc[j]), ("CRC word of row", k, "of", g, "as", q)


# ---- the collision constructions the tests share ----
CRC_POLY = bytes([0x41, 0x06, 0x71, 0xDB, 0x01])              # the CRC-32 polynomial as five message bytes: XORed in anywhere, it keeps zlib's crc32


def crc_twin(buf, at):
    """buf with CRC_POLY XORed in at byte ``at``: other bytes, the same CRC-32 of every stretch that holds the five bytes"""
    out = bytearray(buf)
    for i, x in enumerate(CRC_POLY):
        out[at + i] ^= x
    return bytes(out)


def same_ends(bufs, B):
    """bufs (one length) with the first and the last min(16, block) bytes of every block forced to those of bufs[0]"""
    out = []
    for b in bufs:
        b = bytearray(b)
        for at in range(0, len(b), B):
            e = min(B, len(b) - at)
            k = min(16, e)
            b[at: at + k] = bufs[0][at: at + k]
            b[at + e - k: at + e] = bufs[0][at + e - k: at + e]
        out.append(bytes(b))
    return out


# ---- the cases the CPU and the GPU tests share ----
EMPTY = 0                                                      # row of R.RECIPES; the last one, 11, is empty too


def raw_source(bufs, B, spare=2):
    """bufs as a container whose blocks are all stored raw, with `spare` unused table rows, as a source tuple of splice_model"""
    first, off = [0], [0]
    for b in bufs:
        for at in range(0, len(b), B):
            off.append(off[-1] + min(B, len(b) - at))
        first.append(len(off) - 1)
    nbt = len(off) - 1 + spare
    off += [off[-1]] * spare
    return (b"".join(bufs), off[-1], np.array(first, dtype=np.uint64), np.array(off, dtype=np.uint64), [len(b) for b in bufs],
            R.block_crcs(bufs, B, nbt), len(bufs), nbt)


def expect_two_orders(n):
    """rep of two containers that hold the same n buffers, the second in the order ORDER2, the last buffer empty like the first"""
    rep = list(range(n - 1)) + [EMPTY]
    return rep + [rep[k] for k in ORDER2]
