"""The block transcoder (include/mscomp_amd.h, mscomp_amd_transcoder_*) restated over tests/blocks_model.py and the oracle's one-shot codecs:
the rules of the header in their order, the new container, the statuses and the three counts. Not collected as a test."""
import numpy as np

import blocks_model as M
import crc_model

OK, ARG, DATA, BUF = M.OK, M.ARG, M.DATA, M.BUF
LZNT1 = 2
CARRY, ENCODE, RAW = 1, 2, 3
POLY, ONE = 0xEDB88320, 0x80000000


def crc_mul(a, b):
    """a * b mod the CRC polynomial, x^0 in bit 31 (zlib's multmodp)"""
    p = 0
    for _ in range(32):
        if a & ONE:
            p ^= b
        a = (a << 1) & 0xFFFFFFFF
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def crc_xpow(n):
    """x^n mod the CRC polynomial"""
    r, sq = ONE, ONE >> 1
    while n:
        if n & 1:
            r = crc_mul(r, sq)
        sq = crc_mul(sq, sq)
        n >>= 1
    return r


def crc_fold(crcs, lens):
    """the CRC-32 of a run of pieces from the pieces' CRC-32s and lengths alone: XOR of crc_k x^(8 bytes behind piece k)"""
    v, behind = 0, sum(lens)
    for c, n in zip(crcs, lens):
        behind -= n
        v ^= crc_mul(int(c), crc_xpow(8 * behind)) if behind else int(c)
    return v


def walk(image, e, B2):
    """the chunk headers of one compressed-stored LZNT1 block cut at B2: [(start, end)] of every new block's images, or None when the
    images do not tile the stored bytes into ceil(e / 4096) chunks (no byte at or behind len(image) is read)"""
    pos, s, rows = 0, len(image), []
    for at in range(0, e, B2):
        start = pos
        for _ in range((min(B2, e - at) + 4095) // 4096):
            if pos + 2 > s:
                return None
            pos += ((image[pos] | image[pos + 1] << 8) & 0x0FFF) + 3
            if pos > s:
                return None
        rows.append((start, pos))
    return rows if pos == s else None


def transcode(loader, f1, B1, f2, B2, packed, packed_len, block_first, block_off, lengths, block_crc, nbt, nbn, groups_max, new_cap):
    """(packed bytes that were written, new_first [n + 1], new_off [nbn + 1], new_crc [nbn] or None, statuses [n], (carried, decoded, encoded))"""
    assert (f1, B1) != (f2, B2)
    n = len(lengths)
    first, off = [int(x) for x in block_first], [int(x) for x in block_off]
    with_crc = block_crc is not None
    zero_crc = np.zeros(nbn, dtype=np.uint32) if with_crc else None
    # rule 0
    if first[n] > nbt or any(first[r] > first[r + 1] for r in range(n)):
        return b"", np.zeros(n + 1, dtype=np.uint64), np.zeros(nbn + 1, dtype=np.uint64), zero_crc, np.full(n, ARG, dtype=np.int32), (0, 0, 0)
    G = max(B1, B2)
    mode = "generic" if f1 != LZNT1 or f2 != LZNT1 else "join" if B2 > B1 else "split"
    status, plans, run_rows, run_work = [], [], 0, 0
    for r in range(n):
        L = int(lengths[r])
        run_rows += (L + B2 - 1) // B2
        if first[r + 1] - first[r] != (L + B1 - 1) // B1:                      # rule 1
            status.append(DATA); plans.append(None)
            continue
        if run_rows > nbn:                                                     # rule 2
            status.append(ARG); plans.append(None)
            continue
        # rule 3: the groups of the resource, each (worked, members [(row, o0, o1, e)], new rows [(kind, e2, start, end)])
        groups, bad = [], False
        for at in range(0, L, G):
            span = min(G, L - at)
            members, all_comp = [], True
            for m_at in range(0, span, B1):
                j = first[r] + (at + m_at) // B1
                e, o0, o1 = min(B1, span - m_at), off[j], off[j + 1]
                if o1 < o0 or o1 > packed_len or o1 == o0 or o1 - o0 > e:
                    bad = True
                all_comp = all_comp and o1 - o0 < e
                members.append((j, o0, o1, e))
            if bad:
                break
            new_e = [min(B2, span - k) for k in range(0, span, B2)]
            if mode == "join" and all_comp:
                groups.append((False, members, [(CARRY, span, members[0][1], members[-1][2])]))
            elif mode == "split" and all_comp:
                _, o0, o1, e = members[0]
                tiles = walk(bytes(packed[o0:o1]), e, B2)
                if tiles is None:
                    bad = True
                    break
                rows = [(CARRY, e2, o0 + a, o0 + b) if b - a < e2 else (RAW, e2, 0, 0) for e2, (a, b) in zip(new_e, tiles)]
                groups.append((with_crc or any(k == RAW for k, _, _, _ in rows), members, rows))
            else:
                groups.append((True, members, [(ENCODE, e2, 0, 0) for e2 in new_e]))
        if bad:
            status.append(DATA); plans.append(None)
            continue
        run_work += sum(1 for w, _, _ in groups if w)                          # rule 4
        status.append(ARG if run_work > groups_max else OK)
        plans.append(groups if run_work <= groups_max else None)
    # the worked groups, rule 5, the new tables, rule 6
    carried = decoded = encoded = 0
    new_first, new_off, new_crc, pieces = [0], [0], [], []
    for r in range(n):
        rows_r, crc_r, carried_r = [], [], 0
        for worked, members, rows in plans[r] or []:
            data = None
            if worked:
                data = b""
                for j, o0, o1, e in members:
                    if o1 - o0 == e:
                        data += bytes(packed[o0:o1])
                        continue
                    decoded += 1
                    ds, got, _ = loader.oracle_decompress_ex(f1, bytes(packed[o0:o1]), e)
                    if ds != OK or len(got) != e or (with_crc and crc_model.crc(got) != int(block_crc[j])):
                        status[r] = DATA
                        got = bytes(e)
                    data += got
                encoded += sum(1 for k, _, _, _ in rows if k == ENCODE)
            at = 0
            for kind, e2, a, b in rows:
                if kind == CARRY:
                    rows_r.append(bytes(packed[a:b])); carried_r += 1
                    if with_crc:
                        crc_r.append(crc_fold([block_crc[j] for j, _, _, _ in members], [e for _, _, _, e in members]) if mode == "join"
                                     else crc_model.crc(data[at: at + e2]))
                else:
                    blk = data[at: at + e2]
                    rows_r.append(M.stored(loader, f2, blk) if kind == ENCODE else blk)
                    crc_r.append(crc_model.crc(blk))
                at += e2
        if status[r] != OK:
            rows_r, crc_r, carried_r = [], [], 0
        carried += carried_r
        for s in rows_r:
            new_off.append(new_off[-1] + len(s))
            if new_off[-1] <= new_cap:
                pieces.append(s)
            else:
                status[r] = BUF
        new_crc += crc_r
        new_first.append(len(new_off) - 1)
    new_off += [new_off[-1]] * (nbn + 1 - len(new_off))
    if with_crc:
        zero_crc[: len(new_crc)] = new_crc
    return (b"".join(pieces), np.array(new_first, dtype=np.uint64), np.array(new_off, dtype=np.uint64), zero_crc, np.array(status, dtype=np.int32),
            (carried, decoded, encoded))


def fresh(loader, fmt, buffers, B, with_crc):
    """what mscomp_amd_blocks_compress and mscomp_amd_blocks_crc write for the buffers: (packed, first, off [nb + 1], crc [nb] or None)"""
    total = sum(len(b) for b in buffers)
    packed, first, off, st = M.model_compress(loader, fmt, buffers, B, total, total)
    assert all(int(s) == OK for s in st)
    nb = int(first[len(buffers)])
    crc = crc_model.blocks(buffers, B, total)[0][:nb] if with_crc else None
    return packed, first, off[: nb + 1], crc
