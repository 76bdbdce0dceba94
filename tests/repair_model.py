"""Salvage and repair (include/mscomp_amd.h, mscomp_amd_blocks_salvage and mscomp_amd_deduper_repair) restated in plain Python over
tests/blocks_model.py, zlib's crc32 and the oracle's decoders, and the damage recipes the CPU and the GPU tests share. Not collected as a
test.

A source is the tuple the other models take: (packed, packed_len, first, off, lens, crc or None, n_res, n_blocks_table). A damage recipe
is a function (shape, oracle) -> edits: ``shape`` has the attributes fmt, B, packed, first, off, lens, crc, n, nbt of a healthy container
of R.buffers(B) -- a blocks_rig.Container, or shape_of() on the CPU --, ``edits`` names what the damaged copy states instead
(packed / first / off / lens / crc, and caps: the output capacities of a salvage).
"""
import types
import zlib

import numpy as np

import blocks_model as M
import blocks_rig as G
import extents_model as X
import read_model as R

OK, ARG, DATA, BUF = M.OK, M.ARG, M.DATA, M.BUF
M64 = M.M64
GOOD, TABLE, DECODE, CRC, SKIPPED = 0, 1, 2, 3, 4
BAD = (TABLE, DECODE, CRC)
CAUSES = ("decreasing", "beyond", "s>e", "s=0")                 # why a row is TABLE
ONE, SHORT_TEXT, RANDOM1, TEXT_B1, MIXED, ZEROS5, TEXT, RANDOM3, MIXED5, ZEROS1, LAST = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11   # rows of R.RECIPES


# ---- salvage ------------------------------------------------------------------------------------------------------------------------------
def table_cause(o0, o1, e, packed_len):
    """why decompress's step 4 refuses a row by its table entries, or None"""
    if o1 < o0:
        return "decreasing"
    if o1 > packed_len:
        return "beyond"
    if o1 - o0 > e:
        return "s>e"
    return "s=0" if o1 == o0 else None


def model_salvage(loader, fmt, src, B, in_total_max, out_caps, with_crc=True, only=None):
    """{"verdict" [n_blocks_max], "bad", "out_len", "status" [n_res], "count" [4], "rows": per resource None (refused) or a list of
    (verdict, bytes written or None for a row left alone, cause of a TABLE verdict), "stored": per row the raw-or-compressed form it was
    judged in ("raw" / "compressed" / None)}. A judged row's bytes come from model_decompress asked for that one block."""
    packed, plen, first, off, lens, crc, n, _ = src
    crc = crc if with_crc else None
    nbmax = n + in_total_max // B
    first, off = [int(x) for x in first], [int(x) for x in off]
    verdict, stored = [SKIPPED] * nbmax, [None] * nbmax
    bad, out_len, status, rows, count, run = [], [], [], [], [0, 0, 0, 0], 0
    for r in range(n):
        L = int(lens[r])
        run += L
        nblk = (L + B - 1) // B
        st = OK
        if run > in_total_max or first[r] > nbmax or first[r + 1] > nbmax:
            st = ARG
        elif (first[r + 1] - first[r]) & M64 != nblk:
            st = DATA
        elif L > int(out_caps[r]):
            st = BUF
        if st != OK:
            bad.append(0); out_len.append(0); status.append(st); rows.append(None)
            continue
        mine, nbad = [], 0
        for k in range(nblk):
            j, e = first[r] + k, min(B, L - k * B)
            if only is not None and int(only[j]) == GOOD:
                mine.append((SKIPPED, None, None))
                continue
            cause = table_cause(off[j], off[j + 1], e, plen)
            v, data = GOOD, None
            if cause:
                v = TABLE
            else:
                stored[j] = "raw" if off[j + 1] - off[j] == e else "compressed"
                ranges = [(k, 1) if q == r else (0, 0) for q in range(n)]
                outs, sts = M.model_decompress(loader, fmt, packed, plen, first, off, lens, B, in_total_max, out_caps, ranges)
                if sts[r] != OK:
                    v = DECODE
                else:
                    data = outs[r]
                    assert len(data) == e
                    if crc is not None and zlib.crc32(data) != int(crc[j]):
                        v = CRC
            verdict[j] = v
            count[0] += 1
            if v != GOOD:
                nbad += 1; count[1] += 1; count[2] += e
                data = bytes(e)
            mine.append((v, data, cause))
        count[3] += 1 if nbad else 0
        bad.append(nbad); out_len.append(L); status.append(DATA if nbad else OK); rows.append(mine)
    return {"verdict": np.array(verdict, dtype=np.uint32), "bad": bad, "out_len": out_len, "status": status, "count": count, "rows": rows,
            "stored": stored}


def image_pieces(mo, out_off, B):
    """(offset, bytes) of everything a salvage writes into d_out, for blocks_rig.same_image"""
    return [(int(out_off[r]) + k * B, data) for r, mine in enumerate(mo["rows"]) if mine for k, (_, data, _) in enumerate(mine) if data]


# ---- repair -------------------------------------------------------------------------------------------------------------------------------
def _rule1(src, r, B):
    _, _, first, _, lens, _, _, nbt = src
    f0, f1, L = int(first[r]), int(first[r + 1]), int(lens[r])
    if f0 > f1 or f1 > int(nbt):
        return ARG, 0
    return (OK, f1 - f0) if f1 - f0 == L // B + (1 if L % B else 0) else (DATA, 0)


def model_repair(sources, verdicts, B, n_res, n_blocks_new, with_crc=True):
    """{"ext_first" [n_res + 1], "ext": list of (c, r, k0, count), "fixed", "lost", "status" [n_res], "count" [4], "choice": per resource
    the list of (c, lost)}"""
    with_crc = with_crc and all(s[5] is not None for s in sources)
    p = sources[0]
    ext_first, ext, fixed, lost, status, choice, count, run = [0], [], [], [], [], [], [0, 0, 0, 0], 0
    for r in range(n_res):
        st, n = (ARG, 0) if r >= int(p[6]) else _rule1(p, r, B)
        if st == OK:
            run = min(run + n, M64)
            if n and run > n_blocks_new:
                st, n = ARG, 0
        cs = []
        for k in range(n if st == OK else 0):
            j0, c = int(p[2][r]) + k, None
            for s, src in enumerate(sources):
                if s and (r >= int(src[6]) or _rule1(src, r, B)[0] != OK or int(src[4][r]) != int(p[4][r])):
                    continue
                j = int(src[2][r]) + k
                if int(verdicts[s][j]) == GOOD and (s == 0 or not with_crc or int(src[5][j]) == int(p[5][j0])):
                    c = s
                    break
            cs.append((c or 0, c is None))
            if c:
                count[2] += (int(sources[c][3][int(sources[c][2][r]) + k + 1]) - int(sources[c][3][int(sources[c][2][r]) + k])) & M64
        for k, (c, _) in enumerate(cs):
            if k == 0 or cs[k - 1][0] != c:
                ext.append([c, r, k, 0])
            ext[-1][3] += 1
        nf, nl = sum(1 for c, _ in cs if c), sum(1 for _, gone in cs if gone)
        count[0] += nf; count[1] += nl; count[3] += 1 if nl else 0
        fixed.append(nf); lost.append(nl); status.append(DATA if st == OK and nl else st); choice.append(cs)
        ext_first.append(len(ext))
    return {"ext_first": ext_first, "ext": [tuple(e) for e in ext], "fixed": fixed, "lost": lost, "status": status, "count": count, "choice": choice}


def model_rebuild(sources, mo, B, with_crc=True, n_ext=None, cap=None):
    """the container mscomp_amd_splicer_splice_extents writes from a repair's lists over the same sources: the primary's shape"""
    nbt, room = int(sources[0][7]), sum(int(s[1]) for s in sources)
    return X.model_splice_extents(sources, mo["ext_first"], mo["ext"], B, max(1, len(mo["ext"])) if n_ext is None else n_ext, nbt,
                                  room if cap is None else cap, with_crc=with_crc)


def holds_consequence(sources, mo, B, healthy, with_crc=True):
    """the header's consequence: the rebuilt container has the primary's shape, and with nothing lost and nothing refused it is the
    undamaged container byte for byte -- packed bytes, both tables and the checksums. Returns the rebuilt container."""
    got = model_rebuild(sources, mo, B, with_crc)
    nb = int(healthy[2][-1])
    if not any(mo["status"]):
        assert got["status"] == [OK] * len(mo["status"]) and got["new_len"] == [int(x) for x in healthy[4]]
        assert got["packed"] == bytes(healthy[0]) and np.array_equal(got["first"], healthy[2]) and np.array_equal(got["off"], healthy[3])
        assert not with_crc or np.array_equal(got["crc"][:nb], np.asarray(healthy[5])[:nb])
    return got


# ---- the damage recipes -------------------------------------------------------------------------------------------------------------------
def shape_of(loader, fmt, B):
    """the healthy container of R.buffers(B) as the container model writes it, with the attributes a recipe reads"""
    bufs = R.buffers(B)
    packed, plen, first, off, lens, crc, n, nbt = X.source(loader, fmt, B, bufs)
    return types.SimpleNamespace(fmt=fmt, B=B, bufs=bufs, packed=bytes(packed), plen=plen, first=first, off=off, lens=lens, crc=crc, n=n, nbt=nbt,
                                 total=sum(lens))


def source_of(shape, edits=None):
    """the model's source tuple of a shape with a recipe's edits applied"""
    e = edits or {}
    packed = e.get("packed", shape.packed)
    return (packed, len(packed), np.array(e.get("first", shape.first), dtype=np.uint64), np.array(e.get("off", shape.off), dtype=np.uint64),
            [int(x) for x in e.get("lens", shape.lens)], np.array(e.get("crc", shape.crc), dtype=np.uint32), shape.n, shape.nbt)


def row(shape, r, k=0):
    return int(shape.first[r]) + k


def data_len(shape, r, k):
    return min(shape.B, shape.lens[r] - k * shape.B)


def _flips(shape, oracle, spots):
    """packed with one byte flipped per (resource, block, decodes): G.flip's byte (None: the 6th byte of a raw block)"""
    packed = bytearray(shape.packed)
    for r, k, decodes in spots:
        j = row(shape, r, k)
        at = int(shape.off[j]) + min(5, int(shape.off[j + 1] - shape.off[j]) - 1) if decodes is None else G.flip(oracle, shape, j, data_len(shape, r, k), decodes)
        packed[at] ^= 0xFF if decodes is None else 0x01
    return bytes(packed)


def _off(shape, changes):
    off = np.array(shape.off, dtype=np.uint64)
    for j, v in changes:
        off[j] = v
    return off


def _crc(shape, rows):
    crc = np.array(shape.crc, dtype=np.uint32)
    for j in rows:
        crc[j] ^= 0x80000001
    return crc


def r_decode(s, o):
    return {"packed": _flips(s, o, [(TEXT, 1, False), (SHORT_TEXT, 0, False)])}


def r_crc_compressed(s, o):
    return {"packed": _flips(s, o, [(TEXT, 2, True), (TEXT_B1, 0, True)])}


def r_crc_raw(s, o):
    return {"packed": _flips(s, o, [(RANDOM3, 1, None), (ONE, 0, None), (RANDOM3, 3, None)])}


def r_crc_word(s, o):
    return {"crc": _crc(s, [row(s, MIXED5, 3), row(s, ZEROS5, 0)])}


def r_table_decreasing(s, o):                                  # two raw blocks: row 0 decreases, row 1 then spans both (s > e)
    j = row(s, RANDOM3, 0)
    return {"off": _off(s, [(j + 1, int(s.off[j]) - 1)])}


def r_table_beyond(s, o):                                      # the last block of the container ends behind the stored bytes
    nb = int(s.first[-1])
    return {"off": _off(s, [(nb, int(s.off[nb]) + 5)])}


def r_table_zero(s, o):                                        # a raw block of no stored bytes; the block behind it then spans both (s > e)
    j = row(s, MIXED, 0)
    return {"off": _off(s, [(j + 1, int(s.off[j]))])}


def r_table_and_crc(s, o):                                     # TABLE comes first
    return dict(r_table_zero(s, o), crc=_crc(s, [row(s, MIXED, 0), row(s, MIXED, 1)]))


def r_everything(s, o):
    j, nb = row(s, MIXED, 0), int(s.first[-1])
    return {"packed": _flips(s, o, [(TEXT, 1, False), (TEXT, 2, True), (RANDOM3, 1, None)]), "off": _off(s, [(j + 1, int(s.off[j])), (nb, int(s.off[nb]) + 5)]),
            "crc": _crc(s, [row(s, MIXED5, 3)])}


def r_refused(s, o):                                           # a resource refused by each of rules 1-3 beside damaged ones
    lens, caps, first = list(s.lens), list(s.lens), np.array(s.first, dtype=np.uint64)
    lens[TEXT] = 17                                            # rule 2: four blocks in the table, one by its length
    caps[MIXED5] -= 1                                          # rule 3
    first[-1] = s.nbt + 1                                      # rule 1: the last resource's end lies beyond n_blocks_max
    return {"packed": _flips(s, o, [(SHORT_TEXT, 0, False), (RANDOM3, 1, None)]), "lens": lens, "caps": caps, "first": first}


RECIPES = {"decode": r_decode, "crc_compressed": r_crc_compressed, "crc_raw": r_crc_raw, "crc_word": r_crc_word, "table_decreasing": r_table_decreasing,
           "table_beyond": r_table_beyond, "table_zero": r_table_zero, "table_and_crc": r_table_and_crc, "everything": r_everything, "refused": r_refused}


# the repair case: a primary and two mirrors, damaged in other rows, in one shared row (lost), mirror 2 with a resource of another length
def r_mendable(s, o):                                          # stored bytes and offset entries, no CRC word: a healthy mirror mends all of it
    j, nb = row(s, MIXED, 0), int(s.first[-1])
    return {"packed": _flips(s, o, [(TEXT, 1, False), (TEXT, 2, True), (RANDOM3, 1, None)]), "off": _off(s, [(j + 1, int(s.off[j])), (nb, int(s.off[nb]) + 5)])}


def r_primary(s, o):                                           # (the damaged CRC word of ZEROS5 4 is in no mirror: lost)
    return {"packed": _flips(s, o, [(TEXT, 1, False), (TEXT, 2, True), (RANDOM3, 1, None), (MIXED5, 1, False), (MIXED5, 3, False), (SHORT_TEXT, 0, False)]),
            "crc": _crc(s, [row(s, ZEROS5, 4)])}


def r_mirror1(s, o):                                           # lacks TEXT 1 (the shared row), RANDOM3 1 and MIXED5 3, has the rest
    return {"packed": _flips(s, o, [(TEXT, 1, True), (RANDOM3, 1, None), (MIXED5, 3, False), (MIXED, 1, False)])}


def r_mirror2(s, o):                                           # lacks TEXT 1 too; MIXED5 has another length there: never a candidate for MIXED5 3
    lens = list(s.lens)
    lens[MIXED5] -= 1
    return {"packed": _flips(s, o, [(TEXT, 1, False), (TEXT_B1, 0, False)]), "lens": lens}


REPAIR_CASE = (r_primary, r_mirror1, r_mirror2)
