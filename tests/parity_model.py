"""Parity rows (include/mscomp_amd.h, mscomp_amd_parity_build and mscomp_amd_parity_rebuild) restated in numpy: GF(2^8) by log / antilog
tables built here from the polynomial 0x11D, the code by its DEFINING sum (the library computes it by Horner), the solver by a plain
Gauss-Jordan elimination (the library inverts by cofactors), zlib's crc32 for the parity rows' checksums. Not collected as a test.

A source is the tuple the other models take: (packed, packed_len, first, off, lens, crc or None, n_res, n_blocks_table). A parity set is
a dict {"par": bytes, "par_off", "par_crc", "row_len", "head"} as build writes it (model_build's answer holds one under "set").
"""
import zlib

import numpy as np

import blocks_model as M

OK, ARG, DATA, BUF = M.OK, M.ARG, M.DATA, M.BUF
GOOD, SKIPPED = 0, 4
POLY = 0x11D
K_MAX, M_MAX = 255, 3


def _tables():
    exp, log, x = np.zeros(510, dtype=np.int64), np.zeros(256, dtype=np.int64), 1
    for i in range(255):
        exp[i] = exp[i + 255] = x
        log[x] = i
        x <<= 1
        if x & 0x100:
            x ^= POLY
    return exp, log


EXP, LOG = _tables()


def mul(a, b):
    """the product of two arrays (or numbers) of field elements, by logarithms"""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    return np.where((a == 0) | (b == 0), 0, EXP[LOG[a] + LOG[b]])


def inv(a):
    assert a != 0
    return int(EXP[(255 - LOG[a]) % 255])


def coef(p, i):
    """alpha^(p i): the weight of member i in parity p"""
    return int(EXP[(p * i) % 255])


def x2_packed(v):
    """the library's "times alpha" on four bytes packed in a dword (csrc/gfmath.h gf_x2)"""
    v = int(v) & 0xFFFFFFFF
    return (((v & 0x7F7F7F7F) << 1) ^ (((v >> 7) & 0x01010101) * 0x1D)) & 0xFFFFFFFF


def defining(rows, m):
    """P_p = XOR_i alpha^(p i) D_i over equally long uint8 rows: m parity rows"""
    n = len(rows[0]) if rows else 0
    out = np.zeros((m, n), dtype=np.int64)
    for p in range(m):
        for i, d in enumerate(rows):
            out[p] ^= mul(coef(p, i), d)
    return out.astype(np.uint8)


def horner(rows, m):
    """the same by Horner from the last member down, acc_p = alpha^p acc_p ^ d, with the packed "times alpha" alone"""
    n = len(rows[0]) if rows else 0
    assert n % 4 == 0
    acc = [[0] * (n // 4) for _ in range(m)]
    for d in reversed(rows):
        words = np.frombuffer(np.asarray(d, dtype=np.uint8).tobytes(), dtype="<u4")
        for p in range(m):
            for w in range(n // 4):
                a = acc[p][w]
                for _ in range(p):
                    a = x2_packed(a)
                acc[p][w] = a ^ int(words[w])
    return np.array([np.frombuffer(np.array(a, dtype="<u4").tobytes(), dtype=np.uint8) for a in acc], dtype=np.uint8).reshape(m, n)


def invert(a):
    """the inverse of a square matrix (list of lists) by Gauss-Jordan; None when it is singular"""
    e = len(a)
    a = [list(r) + [1 if i == j else 0 for j in range(e)] for i, r in enumerate(a)]
    for c in range(e):
        piv = next((r for r in range(c, e) if a[r][c]), None)
        if piv is None:
            return None
        a[c], a[piv] = a[piv], a[c]
        d = inv(a[c][c])
        a[c] = [int(mul(x, d)) for x in a[c]]
        for r in range(e):
            if r != c and a[r][c]:
                f = a[r][c]
                a[r] = [x ^ int(mul(f, y)) for x, y in zip(a[r], a[c])]
    return [r[e:] for r in a]


# ---- the two calls ------------------------------------------------------------------------------------------------------------------------
def geometry(nbt, k, m):
    gmax = (nbt + k - 1) // k
    return gmax, gmax * m


def _row_len(src, B, nb, nbt):
    _, plen, _, off, _, _, _, _ = src
    out = np.zeros(nbt, dtype=np.uint32)
    for j in range(nb):
        a, b = int(off[j]), int(off[j + 1])
        if a <= b <= plen and b - a <= B:
            out[j] = b - a
    return out


def _padded(src, j, n, length):
    packed, off = src[0], src[3]
    a = int(off[j])
    d = np.zeros(length, dtype=np.uint8)
    d[:n] = np.frombuffer(bytes(packed[a: a + n]), dtype=np.uint8)
    return d


def _plens(row_len, nb, G, k):
    return [(max(int(row_len[j]) for j in range(g, nb, G)) + 15) // 16 * 16 for g in range(G)]


def model_build(src, B, k, m, par_cap, nbt=None):
    """{"status", "head" [4], "par_off" [m G_max + 1], "par_crc" [m G_max], "row_len" [nbt], "pieces": (offset, bytes) of every parity row
    written, "set": the parity set}; an array the call leaves alone is None."""
    n, nbt = int(src[6]), int(src[7]) if nbt is None else nbt
    gmax, Q = geometry(nbt, k, m)
    nb = int(src[2][n]) if n else 0
    if nb > nbt or int(src[7]) != nbt:
        return {"status": ARG, "head": [0, 0, 0, 0], "par_off": [0] * (Q + 1) if nbt else None, "par_crc": None, "row_len": None, "pieces": [], "set": None}
    if nbt == 0:
        return {"status": OK, "head": [0, 0, k, m], "par_off": None, "par_crc": None, "row_len": None, "pieces": [], "set": None}
    row_len = _row_len(src, B, nb, nbt)
    G = (nb + k - 1) // k
    plens = _plens(row_len, nb, G, k)
    par_off, par_crc, pieces, status = [0], [0] * Q, [], OK
    for g in range(G):
        rows = [_padded(src, j, int(row_len[j]), plens[g]) for j in range(g, nb, G)]
        par = defining(rows, m)
        for p in range(m):
            par_off.append(par_off[-1] + plens[g])
            if par_off[-1] <= par_cap:
                pieces.append((par_off[-2], par[p].tobytes()))
                par_crc[g * m + p] = zlib.crc32(par[p].tobytes())
            else:
                status = BUF
    par_off += [par_off[-1]] * (Q + 1 - len(par_off))
    image = bytearray(par_off[-1])
    for at, b in pieces:
        image[at: at + len(b)] = b
    pset = {"par": bytes(image), "par_off": np.array(par_off, dtype=np.uint64), "par_crc": np.array(par_crc, dtype=np.uint32), "row_len": row_len,
            "head": np.array([nb, G, k, m], dtype=np.uint64)}
    return {"status": status, "head": [nb, G, k, m], "par_off": par_off, "par_crc": par_crc, "row_len": [int(x) for x in row_len], "pieces": pieces, "set": pset}


def model_rebuild(src, verdict, pset, B, k, m, fix_cap, nbt=None, par_len=None):
    """{"status", "count" [6], "fix_off" [nbt + 1], "fix_verdict" [nbt], "pieces": (offset, bytes) of every rebuilt row written, "rebuilt":
    the rows rebuilt, "unrecoverable": the groups, "used": per damaged recoverable group the parities used}; None: left alone."""
    n, nbt = int(src[6]), int(src[7]) if nbt is None else nbt
    _, plen, _, off, _, _, _, _ = src
    nb = int(src[2][n]) if n else 0
    par, par_off, par_crc, row_len, head = pset["par"], pset["par_off"], pset["par_crc"], pset["row_len"], [int(x) for x in pset["head"]]
    par_len = len(par) if par_len is None else par_len
    refused = lambda st: {"status": st, "count": [0] * 6, "fix_off": [0] * (nbt + 1) if nbt else None, "fix_verdict": [SKIPPED] * nbt, "pieces": [],
                          "rebuilt": [], "unrecoverable": [], "used": {}}
    if nb > nbt or int(src[7]) != nbt:
        return refused(ARG)
    G = (nb + k - 1) // k
    if head != [nb, G, k, m]:
        return refused(DATA)
    if nbt == 0:
        return dict(refused(OK), fix_off=None)
    present = [int(verdict[j]) == GOOD and int(off[j]) <= int(off[j + 1]) <= plen and int(off[j + 1]) - int(off[j]) == int(row_len[j]) for j in range(nb)]
    plens = _plens(row_len, nb, G, k)
    count, fixlen, data, unrec, used = [0] * 6, [0] * nbt, {}, [], {}
    for g in range(G):
        usable = []
        for p in range(m):
            q = g * m + p
            a, b = int(par_off[q]), int(par_off[q + 1])
            if a <= b <= par_len and a % 16 == 0 and b - a == plens[g] and zlib.crc32(bytes(par[a:b])) == int(par_crc[q]):
                usable.append(p)
        count[4] += m - len(usable)
        members = list(range(g, nb, G))
        missing = [i for i, j in enumerate(members) if not present[j]]
        if not missing:
            continue
        count[0] += len(missing); count[2] += 1
        if len(missing) > len(usable):
            count[3] += 1; unrec.append(g)
            continue
        ps = usable[: len(missing)]
        used[g] = ps
        rows = [_padded(src, j, int(row_len[j]), plens[g]) if present[j] else np.zeros(plens[g], dtype=np.uint8) for j in members]
        syn = defining(rows, m)
        s = [syn[p].astype(np.int64) ^ np.frombuffer(bytes(par[int(par_off[g * m + p]): int(par_off[g * m + p]) + plens[g]]), dtype=np.uint8) for p in ps]
        ai = invert([[coef(p, i) for i in missing] for p in ps])
        assert ai is not None
        for b, i in enumerate(missing):
            d = np.zeros(plens[g], dtype=np.int64)
            for a in range(len(ps)):
                d ^= mul(ai[b][a], s[a])
            j = members[i]
            fixlen[j] = int(row_len[j])
            data[j] = d.astype(np.uint8).tobytes()[: fixlen[j]]
            count[1] += 1; count[5] += fixlen[j]
    fix_off, fix_verdict, pieces, status = [0], [SKIPPED] * nbt, [], OK
    for j in range(nbt):
        fix_off.append(fix_off[-1] + fixlen[j])
        if j in data:
            if fix_off[-1] <= fix_cap:
                pieces.append((fix_off[-2], data[j])); fix_verdict[j] = GOOD
            else:
                status = BUF
    if status == OK and count[3]:
        status = DATA
    return {"status": status, "count": count, "fix_off": fix_off, "fix_verdict": fix_verdict, "pieces": pieces, "rebuilt": sorted(data), "unrecoverable": unrec,
            "used": used}


def fix_source(src, mo):
    """the sparse mirror a rebuild wrote, as a source beside ``src``: its first, lens and crc with the fix's stored bytes and offsets"""
    total = int(mo["fix_off"][-1])
    image = bytearray(total)
    for at, b in mo["pieces"]:
        image[at: at + len(b)] = b
    return (bytes(image), total, src[2], np.array(mo["fix_off"], dtype=np.uint64), src[4], src[5], src[6], src[7])
