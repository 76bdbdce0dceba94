"""The writer's resize (include/mscomp_amd.h, mscomp_amd_writer_resize) restated over tests/blocks_model.py, tests/read_model.py and
tests/write_model.py, with the header's rules 0-10 in their order, and mscomp_amd_res_crc_dev restated over zlib.crc32 and the CRC
polynomial. Not collected as a test.
"""
import zlib

import numpy as np

import blocks_model as M

OK, ARG, DATA, BUF = M.OK, M.ARG, M.DATA, M.BUF
POLY, ONE = 0xEDB88320, 0x80000000                             # the reflected CRC-32 polynomial; x^0 as a register


def resized(buffers, want):
    """the resources cut to, or padded with zeros to, the wanted lengths, by plain slicing"""
    return [bytes(b[:w]) + bytes(max(0, w - len(b))) for b, w in zip(buffers, want)]


def geometry(L, W, n, B):
    """(n', the changed block as (k, e, e') or None, cost) of a resource of L bytes in n = ceil(L / B) blocks that is to have W bytes"""
    n2 = W // B + (1 if W % B else 0)
    changed, mn = None, min(n, n2)
    if mn:
        k = mn - 1
        e, e2 = min(B, L - k * B), min(B, W - k * B)
        if e != e2:
            changed = (k, e, e2)
    return n2, changed, (1 if changed else 0) + max(0, n2 - n)


def model_resize(loader, fmt, packed, packed_len, block_first, block_off, lengths, B, n_blocks_table, want, blocks_max, new_cap, block_crc=None):
    """dict: packed (the bytes written: the blocks that end within new_cap), first (n + 1), off (n_blocks_table + 1), crc (n_blocks_table, or
    None), new_len, res_status (per resource), counts (units, changed blocks read, blocks encoded), reached (the rules that decided something)"""
    n, nbt = len(lengths), n_blocks_table
    first, off = [int(x) for x in block_first], [int(x) for x in block_off]
    reached = set()

    def refused(rule):
        reached.add(rule)
        return {"packed": b"", "first": np.zeros(n + 1, dtype=np.uint64), "off": np.zeros(nbt + 1, dtype=np.uint64),
                "crc": None if block_crc is None else np.zeros(nbt, dtype=np.uint32), "new_len": [0] * n, "res_status": [ARG] * n,
                "counts": (0, 0, 0), "reached": reached}
    if first[n] > nbt or any(first[i] > first[i + 1] for i in range(n)):    # 0. the table as a whole
        return refused(0)

    def block(j, e):                                           # a block's data by the writer's rule 5, or None
        o0, o1 = off[j], off[j + 1]
        if o1 < o0 or o1 > packed_len or o1 - o0 > e or o1 == o0:
            return None
        if o1 - o0 == e:
            data = bytes(packed[o0:o1])
        else:
            ds, got, _ = loader.oracle_decompress_ex(fmt, bytes(packed[o0:o1]), e)
            data = got if ds == OK and len(got) == e else None
        if data is not None and block_crc is not None and zlib.crc32(data) != int(block_crc[j]):
            data = None
        return data
    status, plans, run, units, read, encoded = [], [], 0, 0, 0, 0
    for r in range(n):
        L, W, cnt = int(lengths[r]), int(want[r]), first[r + 1] - first[r]
        st, plan = OK, None
        if cnt != (L + B - 1) // B:                             # 1. block count
            st = DATA; reached.add(1)
        elif W == L:                                           # 2. no change
            reached.add(2)
        else:
            n2, changed, cost = geometry(L, W, cnt, B)
            run += cost                                        # 3. the budget: refused resources stay in the sum
            if run > blocks_max:
                st = ARG; reached.add(3)
            else:
                units += cost
                data = b""
                if changed:                                    # 4. readable
                    read += 1
                    data = block(first[r] + changed[0], changed[1])
                    if data is None:
                        st = DATA; reached.add(4)
                if st == OK:
                    plan = (n2, changed, data)
                    encoded += cost
        if st != OK:
            reached.add(5)                                     # 5. carried
        status.append(st)
        plans.append(plan)
    zeros = {}                                                 # the stored form of e zero bytes: made once per length

    def stored(d):
        if not any(d):
            if len(d) not in zeros:
                zeros[len(d)] = M.stored(loader, fmt, d)
            return zeros[len(d)]
        return M.stored(loader, fmt, d)
    rows, new_first, new_len = [], [0], []                     # rows: (stored bytes, checksum) per NEW table row
    for r in range(n):
        L, W, cnt = int(lengths[r]), int(want[r]), first[r + 1] - first[r]
        n2, changed, data = plans[r] if plans[r] else (cnt, None, b"")
        for k in range(n2):
            d = None
            if changed and k == changed[0]:                    # 6. new data: kept bytes, then zeros
                keep = min(changed[1], changed[2])
                d = data[:keep] + bytes(changed[2] - keep)
            elif k >= cnt:
                d = bytes(min(B, W - k * B))
            if d is not None:
                reached.add(6)
                rows.append((stored(d), zlib.crc32(d)))
            else:                                              # 7. clean: verbatim, an unreadable entry becomes empty
                reached.add(7)
                j = first[r] + k
                s = bytes(packed[off[j]: off[j + 1]]) if off[j] <= off[j + 1] <= packed_len else b""
                rows.append((s, 0 if block_crc is None else int(block_crc[j])))
        new_first.append(len(rows))
        new_len.append(W if plans[r] else L)
    if len(rows) > nbt:                                        # 8. room in the table, on the final counts
        return refused(8)
    reached.add(9)                                             # 9. the tables
    new_off, pieces = [0], []
    for s, _ in rows:
        new_off.append(new_off[-1] + len(s))
        if new_off[-1] <= new_cap:                             # 10. capacity
            pieces.append(s)
    res_status = []
    for r in range(n):
        over = new_first[r + 1] > new_first[r] and new_off[new_first[r + 1]] > new_cap
        if over:
            reached.add(10)
        res_status.append(BUF if over else status[r])
    new_off += [new_off[-1]] * (nbt + 1 - len(new_off))
    return {"packed": b"".join(pieces), "first": np.array(new_first, dtype=np.uint64), "off": np.array(new_off, dtype=np.uint64),
            "crc": None if block_crc is None else np.array([c for _, c in rows] + [0] * (nbt - len(rows)), dtype=np.uint32),
            "new_len": new_len, "res_status": res_status, "counts": (units, read, encoded), "reached": reached}


def crc_mul(a, b):
    """a * b modulo the CRC polynomial, registers with the coefficient of x^0 in bit 31 (zlib's multmodp)"""
    p = 0
    for _ in range(32):
        if a & ONE:
            p ^= b
        a = (a << 1) & 0xFFFFFFFF
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def crc_xpow(nbits):
    """x^nbits modulo the CRC polynomial"""
    r, sq = ONE, ONE >> 1
    while nbits:
        if nbits & 1:
            r = crc_mul(r, sq)
        sq = crc_mul(sq, sq)
        nbits >>= 1
    return r


def model_res_crc(block_first, lengths, block_crc, B, n_blocks_table):
    """(res_crc uint32 [n], status [n]) as mscomp_amd_res_crc_dev gives them: the XOR over a resource's blocks of their CRC-32 times
    x^(8 bytes of the resource behind the block)"""
    first = [int(x) for x in block_first]
    out, st = [], []
    for r, L in enumerate(int(x) for x in lengths):
        f0, f1 = first[r], first[r + 1]
        if f0 > n_blocks_table or f1 > n_blocks_table:
            out.append(0); st.append(ARG)
        elif (f1 - f0) & M.M64 != (L + B - 1) // B:
            out.append(0); st.append(DATA)
        else:
            c = 0
            for k in range(f1 - f0):
                c ^= crc_mul(int(block_crc[f0 + k]), crc_xpow(8 * (L - min(L, (k + 1) * B))))
            out.append(c); st.append(OK)
    return np.array(out, dtype=np.uint32), st


# ---- the cases the CPU and the GPU tests share ----
SPARE = 16
WANTS = (lambda L, B: 0, lambda L, B: 1, lambda L, B: max(0, L - 1), lambda L, B: L, lambda L, B: L + 1, lambda L, B: L // B * B,
         lambda L, B: (L + B - 1) // B * B, lambda L, B: L + B, lambda L, B: L + 2 * B + 5)


def mixes(lens, B):
    """nine batches of wanted lengths: every resource meets every entry of WANTS once, shrinking and growing ones side by side"""
    return [[WANTS[(r + v) % len(WANTS)](L, B) for r, L in enumerate(lens)] for v in range(len(WANTS))]
